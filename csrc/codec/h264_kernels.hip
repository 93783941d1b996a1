// HIP/CDNA4 kernels of the H.264 encoder.
//
// Decomposition (gfx950: 256 CUs, wave64):
//  * k_me_full      one 256-thread workgroup per macroblock; the search window is staged
//                   in LDS and every lane scores (2R+1)^2/256 integer candidates, four
//                   horizontally adjacent ones per v_qsad_pk_u16_u8, then optional
//                   quarter-pel refinement; block-wide argmin via shuffles + LDS.
//  * k_scroll_probe / k_scroll_decide  (EncoderConfig::scroll_range) one workgroup per probe
//                   macroblock scores the 1-D displacements up to the reach and votes; one
//                   workgroup decides the picture's scroll hint, which the _scroll
//                   instantiations of the search kernels may centre their window on.
//  * k_inter_encode one wave per macroblock (4 per workgroup): motion compensation
//                   (6-tap qpel / bilinear chroma), 4x4 integer transform, quantisation,
//                   reconstruction into the reference frame.  Fully parallel over MBs.  A
//                   macroblock whose residual is known to quantise to zero runs no transform.
//  * k_p_fused      k_me_full and k_inter_encode in one kernel: the workgroup that searched a
//                   macroblock codes it on its wave 0 (P pictures whose search reads the
//                   picture the coder predicts from; the two kernels remain for the others).
//  * k_intra_analyze one wave per MB: open-loop Intra4x4 / Intra16x16 / chroma mode costs
//                   (SATD vs source-neighbour predictions) and the intra / inter decision.
//  * k_intra_wave   one workgroup per MB row (luma wave + chroma wave): closed-loop coding
//                   of the intra MBs in a diagonal wavefront with per-row progress flags.
//  * k_cavlc        one wave per macroblock: lane 0 codes the MB header (P_Skip decision,
//                   median mv prediction, cbp), lanes 1..27 code one residual block each;
//                   a wave prefix-sum places every lane's bits in an LDS slot.
//  * k_scan_rows / k_scan_out  one workgroup per MB row, two passes: skip runs, per-MB and
//                   per-slice bit offsets, the frame's distortion.
//  * k_pack         one thread per output word gathers the overlapping header / MB /
//                   trailer bits and stores the word straight into pinned host memory.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../common/hip_check.h"
#include "../common/wave.h"
#include "h264_core.h"
#include "h264_deblock.h"
#include "h264_gpu.h"
#include "h264_mb.h"

namespace mx {
namespace h264 {

namespace {

__device__ __forceinline__ uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

// ------------------------------------------------------------------ half-pel planes
// LDS-tiled F/H/V/J plane builder, 128x16 output tile per 256-thread workgroup.
//  1. the (16+5)-row clamped sample footprint is staged as whole dwords (aligned start
//     4 samples left of the tile; interior tiles use dword loads, border tiles clamp);
//  2. the horizontal 6-tap intermediates b1 for all 21 rows, 4 columns per item;
//  3. each lane produces a 4-pixel x 2-row block of all four planes from 7 sample dwords
//     and 7 b1 quads it shares between the two rows, and stores dwords (64 lanes = 2 rows
//     x 128 contiguous bytes per plane).
// The byte-per-lane version (64x16 tile) ran 19.6 us at 1080p (profiles/r01_final_check).
constexpr int kHpTW = 128, kHpTH = 16;
constexpr int kHpSW = kHpTW + 8;  // staged samples per row: padded x in [px0-4, px0+kHpTW+4)
__device__ __forceinline__ int byte_of(uint32_t w, int k) { return (int)((w >> (8 * k)) & 0xff); }
// Low bytes of a..d -> one dword via v_perm_b32.  Written as `clip255(v) << 8*j` ORs, the
// build produced 0xff in bytes 2-3 whenever sample 1 clamped from below to 0 (seen on the
// MI355X in test_hpel_planes_match_reference; a codegen issue, most likely in the narrowed
// clamp); v_perm reads only byte 0 of each operand, so stale high bits cannot leak.
__device__ __forceinline__ uint32_t pack4(int a, int b, int c, int d) {
    const uint32_t lo = __builtin_amdgcn_perm((uint32_t)b, (uint32_t)a, 0x0c0c0400u);
    const uint32_t hi = __builtin_amdgcn_perm((uint32_t)d, (uint32_t)c, 0x0c0c0400u);
    return __builtin_amdgcn_perm(hi, lo, 0x05040100u);
}
// Frame-state publication: the first kernel of a frame receives the state by value (kernel
// arguments, no extra dispatch) and stores it for the later kernels, replacing a per-frame
// 4.4 us host->device copy node (profiles/r02_b).  Under hipGraph capture the state still
// comes from a captured memcpy node (the captured argument would be stale), so `publish` = 0
// and the kernel reads the device copy.
struct StateArg {
    FrameState v;
    FrameState* dst;
    int publish;
    uint64_t* t_start;  // OutHeader::t_start of the frame (device), or nullptr
};
__device__ __forceinline__ void publish_state(const StateArg& a) {
    static_assert(sizeof(FrameState) % 4 == 0, "FrameState is copied as dwords");
    if (a.t_start && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *a.t_start = wall_clock64();
    if (a.publish && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < sizeof(FrameState) / 4)
        reinterpret_cast<uint32_t*>(a.dst)[threadIdx.x] = reinterpret_cast<const uint32_t*>(&a.v)[threadIdx.x];
}
__device__ __forceinline__ const FrameState& state_of(const StateArg& a) { return a.publish ? a.v : *a.dst; }
// Host side: the argument of a launch.  publish: the state to pass by value, or nullptr to read
// b.fs; stamp: this kernel is the picture's first and records OutHeader::t_start.
inline StateArg make_state_arg(const DeviceBuffers& b, const FrameState* publish, bool stamp = true) {
    StateArg sa{};
    if (publish) sa.v = *publish;
    sa.dst = b.fs;
    sa.publish = publish ? 1 : 0;
    sa.t_start = (b.out_hdr && stamp) ? &b.out_hdr->t_start : nullptr;
    return sa;
}

__global__ __launch_bounds__(256) void k_hpel(Geometry g, StateArg sa, uint8_t* __restrict__ pf,
                                              uint8_t* __restrict__ ph, uint8_t* __restrict__ pv,
                                              uint8_t* __restrict__ pj, int hp_pitch) {
    __shared__ uint32_t smp[kHpTH + 5][kHpSW / 4];
    __shared__ int4 b1[kHpTH + 5][kHpTW / 4];  // 4 columns per entry
    publish_state(sa);
    const uint8_t* __restrict__ ref = state_of(sa).ref_y;
    const int px0 = blockIdx.x * kHpTW, py0 = blockIdx.y * kHpTH;  // padded-plane coordinates
    const int W = g.coded_w + 2 * kHpelPad, H = g.coded_h + 2 * kHpelPad;
    const int tid = threadIdx.x;
    // smp[r][k] = picture sample (px0 - 4 + k - pad, py0 - 2 + r - pad), clamped to the picture
    const int xs = px0 - 4 - kHpelPad, ys = py0 - 2 - kHpelPad;
    const bool interior = xs >= 0 && xs + kHpSW <= g.coded_w && ys >= 0 && ys + kHpTH + 5 <= g.coded_h &&
                          (g.pitch & 3) == 0 && (reinterpret_cast<uintptr_t>(ref) & 3) == 0;
    for (int i = tid; i < (kHpTH + 5) * (kHpSW / 4); i += 256) {
        const int r = i / (kHpSW / 4), k4 = i - r * (kHpSW / 4);
        uint32_t w;
        if (interior) {
            w = *reinterpret_cast<const uint32_t*>(ref + (size_t)(ys + r) * g.pitch + xs + 4 * k4);
        } else {
            w = 0;
            for (int k = 0; k < 4; ++k)
                w |= (uint32_t)ref_px(ref, g.pitch, g.coded_w, g.coded_h, xs + 4 * k4 + k, ys + r) << (8 * k);
        }
        smp[r][k4] = w;
    }
    __syncthreads();
    // b1 at output column c uses samples k = c+2 .. c+7; a 4-column group c = 4q needs
    // staged dwords q, q+1, q+2
    for (int i = tid; i < (kHpTH + 5) * (kHpTW / 4); i += 256) {
        const int r = i / (kHpTW / 4), q = i - r * (kHpTW / 4);
        const uint32_t w0 = smp[r][q], w1 = smp[r][q + 1], w2 = smp[r][q + 2];
        int s[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s[k] = byte_of(w0, k);
            s[4 + k] = byte_of(w1, k);
            s[8 + k] = byte_of(w2, k);
        }
        int t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = tap6(s[j + 2], s[j + 3], s[j + 4], s[j + 5], s[j + 6], s[j + 7]);
        b1[r][q] = make_int4(t[0], t[1], t[2], t[3]);
    }
    __syncthreads();
    const int q = tid & (kHpTW / 4 - 1), r0 = (tid / (kHpTW / 4)) * 2;  // 32 groups x 8 row pairs
    const int x = px0 + 4 * q;
    if (x >= W) return;  // W % 4 == 0: a group is wholly inside or outside
    // output row r reads staged rows r .. r+5 (centre r+2); the pair shares rows r0+1 .. r0+5
    int sv[7][4], bv[7][4];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const uint32_t w = smp[r0 + k][q + 1];  // samples k = 4q+4 .. 4q+7 = output columns 4q .. 4q+3
        const int4 bb = b1[r0 + k][q];
#pragma unroll
        for (int j = 0; j < 4; ++j) sv[k][j] = byte_of(w, j);
        bv[k][0] = bb.x;
        bv[k][1] = bb.y;
        bv[k][2] = bb.z;
        bv[k][3] = bb.w;
    }
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int y = py0 + r0 + rr;
        if (y >= H) break;
        int Hs[4], Vs[4], Js[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            Hs[j] = clip255((bv[rr + 2][j] + 16) >> 5);  // centre row of this output row: rr + 2
            const int v1 = tap6(sv[rr][j], sv[rr + 1][j], sv[rr + 2][j], sv[rr + 3][j], sv[rr + 4][j], sv[rr + 5][j]);
            Vs[j] = clip255((v1 + 16) >> 5);
            const int j1 = tap6(bv[rr][j], bv[rr + 1][j], bv[rr + 2][j], bv[rr + 3][j], bv[rr + 4][j], bv[rr + 5][j]);
            Js[j] = clip255((j1 + 512) >> 10);
        }
        const size_t o = (size_t)y * hp_pitch + x;
        *reinterpret_cast<uint32_t*>(pf + o) = smp[r0 + rr + 2][q + 1];
        *reinterpret_cast<uint32_t*>(ph + o) = pack4(Hs[0], Hs[1], Hs[2], Hs[3]);
        *reinterpret_cast<uint32_t*>(pv + o) = pack4(Vs[0], Vs[1], Vs[2], Vs[3]);
        *reinterpret_cast<uint32_t*>(pj + o) = pack4(Js[0], Js[1], Js[2], Js[3]);
    }
}

// Quarter-sample luma value from an LDS-staged 18x18 footprint of the four planes
// (sp[0] F, sp[1] H, sp[2] V, sp[3] J; local origin one sample up-left of the integer
// match); Table 8-12 on k_hpel's planes, identical to luma_qpel() on the clamped reference.
constexpr int kSpW = 20;
__device__ __forceinline__ int qpel_lds(const uint8_t (*sp)[18][kSpW], int x4, int y4) {
    const int xi = x4 >> 2, yi = y4 >> 2, xf = x4 & 3, yf = y4 & 3;
    const int G = sp[0][yi][xi];
    if ((xf | yf) == 0) return G;
    if (yf == 0) {
        const int b = sp[1][yi][xi];
        if (xf == 2) return b;
        return ((xf == 1 ? G : (int)sp[0][yi][xi + 1]) + b + 1) >> 1;
    }
    if (xf == 0) {
        const int hh = sp[2][yi][xi];
        if (yf == 2) return hh;
        return ((yf == 1 ? G : (int)sp[0][yi + 1][xi]) + hh + 1) >> 1;
    }
    if (xf == 2 && yf == 2) return sp[3][yi][xi];
    if (xf == 2) return ((yf == 1 ? (int)sp[1][yi][xi] : (int)sp[1][yi + 1][xi]) + sp[3][yi][xi] + 1) >> 1;
    if (yf == 2) return ((xf == 1 ? (int)sp[2][yi][xi] : (int)sp[2][yi][xi + 1]) + sp[3][yi][xi] + 1) >> 1;
    const int bb = (yf == 1) ? sp[1][yi][xi] : sp[1][yi + 1][xi];
    const int hh = (xf == 1) ? sp[2][yi][xi] : sp[2][yi][xi + 1];
    return (bb + hh + 1) >> 1;
}

// ------------------------------------------------------------------ motion estimation
constexpr int kMaxRange = 32;
// The LDS search window holds the edge-clamped reference around the macroblock: the +-R candidate
// positions plus the reach of the six-tap filter around the +-1-sample sub-sample refinement, 3
// samples before and 4 after on each axis (4 before in x: whole dwords).  Window byte (wx, wy) is
// picture sample (x0 - R - kWinPadX + wx, y0 - R - kWinPadY + wy).
constexpr int kWinPadX = 4, kWinPadY = 3;
constexpr int kWinStride = 16 + 2 * kMaxRange + 8;  // bytes per LDS window row: a full row at R = 32
constexpr int kWinRows = 16 + 2 * kMaxRange + 7;
constexpr int kWinWords = kWinRows * kWinStride / 4;

constexpr int kMeThreads = 256, kMeWaves = kMeThreads / 64;
// v_qsad_pk_u16_u8: the SADs of `src` against bytes 0..3, 1..4, 2..5 and 3..6 of the 64-bit window
// hi:lo, each added to its 16-bit field of acc -- four horizontally adjacent candidates at once.
__device__ __forceinline__ uint64_t qsad4(uint32_t hi, uint32_t lo, uint32_t src, uint64_t acc) {
    return __builtin_amdgcn_qsad_pk_u16_u8(((uint64_t)hi << 32) | lo, src, acc);
}
// F / H / V / J footprints (18x18 each, the layout qpel_lds reads) around `n` (1 or 2) integer
// matches, computed from the staged window with k_hpel's arithmetic: unclipped horizontal six-tap
// intermediates b1, H = (b1 + 16) >> 5, V the same from the sample column, J = (six taps over
// the b1 column + 512) >> 10.  org0 / org1: window byte of each footprint's sample (0, 0), one
// sample up-left of the match; its 2 rows / columns before and 3 after are in the window.  The
// whole workgroup calls it (one barrier inside) and synchronises before it reads sp.
constexpr int kFpRows = 18 + 5;
__device__ __forceinline__ void build_footprints(const uint8_t* win, int org0, int org1, int n,
                                                 uint8_t (*sp)[4][18][kSpW], int16_t (*b1)[kFpRows][kSpW], int tid) {
    for (int i = tid; i < n * kFpRows * 18; i += kMeThreads) {
        const int pi = i / (kFpRows * 18), rem = i - pi * (kFpRows * 18), r = rem / 18, c = rem - r * 18;
        const uint8_t* p = win + (pi ? org1 : org0) + (r - 2) * kWinStride + c;
        b1[pi][r][c] = (int16_t)tap6(p[-2], p[-1], p[0], p[1], p[2], p[3]);  // -2550 .. 10710
    }
    __syncthreads();
    for (int i = tid; i < n * 324; i += kMeThreads) {
        const int pi = i / 324, rem = i - pi * 324, r = rem / 18, c = rem - r * 18;
        const uint8_t* p = win + (pi ? org1 : org0) + r * kWinStride + c;
        const int16_t(*b)[kSpW] = b1[pi];
        const int v1 = tap6(p[-2 * kWinStride], p[-kWinStride], p[0], p[kWinStride], p[2 * kWinStride], p[3 * kWinStride]);
        const int j1 = tap6(b[r][c], b[r + 1][c], b[r + 2][c], b[r + 3][c], b[r + 4][c], b[r + 5][c]);
        sp[pi][0][r][c] = p[0];
        sp[pi][1][r][c] = (uint8_t)clip255((b[r + 2][c] + 16) >> 5);
        sp[pi][2][r][c] = (uint8_t)clip255((v1 + 16) >> 5);
        sp[pi][3][r][c] = (uint8_t)clip255((j1 + 512) >> 10);
    }
}

// Four waves.  (Five -- the +-16 search's 297 candidate tasks in one pass of 320 threads instead
// of 1.16 passes of 256 -- measured slower: 45 -> 54 us at 1080p, 78 -> 110 us at 4K, the larger
// workgroups costing more in occupancy than the shorter second pass saved: profiles/r04_h264.)
// What the search reads of the frame state, taken once into scalar registers (a pointer that is
// either the kernel's argument block or the published copy would turn every read into a flat load)
struct MeState {
    const uint8_t* ref;  // the reference picture's luma, before its in-loop filter when it was deblocked
    int qp, search_range, subpel, me_coarse, partitions;
};
__device__ __forceinline__ MeState me_state(const FrameState& f) {
    return MeState{f.me_ref ? f.me_ref : f.ref_y, f.qp, f.search_range, f.subpel, f.me_coarse, f.partitions};
}
// The 16x16 SAD of the zero vector (the static exit), one wave calling (tid < 64): a dword of source
// and of reference per lane, v_sad_u8, summed over the wave.  *sw: this lane's source dword.
__device__ __forceinline__ uint32_t zero_sad_wave(const uint8_t* __restrict__ src_y, const uint8_t* __restrict__ ref,
                                                  int pitch, int x0, int y0, int tid, uint32_t* sw) {
    const int r = tid >> 2, c4 = (tid & 3) * 4;
    *sw = *reinterpret_cast<const uint32_t*>(src_y + (y0 + r) * pitch + x0 + c4);
    const uint32_t rw = *reinterpret_cast<const uint32_t*>(ref + (y0 + r) * pitch + x0 + c4);
    return (uint32_t)wave_sum((int)__builtin_amdgcn_sad_u8(*sw, rw, 0u));
}
__device__ __forceinline__ unsigned long long kmin(unsigned long long a, unsigned long long c) { return c < a ? c : a; }
// The minimum of the kMeWaves per-wave keys a block reduction left in LDS.
__device__ __forceinline__ unsigned long long block_min(const unsigned long long* slot) {
    unsigned long long b = slot[0];
    for (int i = 1; i < kMeWaves; ++i) b = kmin(b, slot[i]);
    return b;
}
// Row r of a scoring task: the five window dwords at win32[a] (a dword-aligned 20-byte span shared by
// the four horizontally adjacent candidates) against the four source dwords of the row.  The left
// and right halves of the row go to lft and rgt: a quadrant pair, or one 16x16 accumulator twice.
__device__ __forceinline__ void me_row(const uint32_t* win32, const uint32_t* srcw, int a, int r, uint64_t& lft,
                                       uint64_t& rgt) {
    const uint32_t w0 = win32[a], w1 = win32[a + 1], w2 = win32[a + 2], w3 = win32[a + 3], w4 = win32[a + 4];
    const uint32_t s0 = srcw[r * 4 + 0], s1 = srcw[r * 4 + 1], s2 = srcw[r * 4 + 2], s3 = srcw[r * 4 + 3];
    lft = qsad4(w1, w0, s0, lft);
    lft = qsad4(w2, w1, s1, lft);
    rgt = qsad4(w3, w2, s2, rgt);
    rgt = qsad4(w4, w3, s3, rgt);
}
// The 16x16 scoring loop.  Task q is dword group q % gw of candidate row q / gw; kCoarse takes every
// second row and shifts 0 and 2 of the group (the even-offset grid), otherwise every row and all four
// shifts.  visit(sad, dxr, dyr) gets each candidate inside the window.
template <bool kCoarse, class Visit>
__device__ __forceinline__ void me_score16(const uint32_t* win32, const uint32_t* srcw, int ntask, int gw, int side,
                                           int tid, Visit visit) {
    constexpr int kStep = kCoarse ? 2 : 1, kUnroll = kCoarse ? 4 : 2;
    for (int q = tid; q < ntask; q += kMeThreads) {
        const int dyr = kStep * (q / gw), g = q % gw;
        uint64_t acc = 0;  // four shifted 16x16 SADs, 16 bits each (<= 65,280)
#pragma unroll kUnroll
        for (int r = 0; r < 16; ++r) me_row(win32, srcw, (dyr + r) * (kWinStride / 4) + g, r, acc, acc);
#pragma unroll
        for (int sh = 0; sh < 4; sh += kStep) {
            const int dxr = 4 * g + sh;
            if (dxr >= side) break;
            visit((uint32_t)(acc >> (16 * sh)) & 0xffffu, dxr, dyr);
        }
    }
}
// One of the 8 integer neighbours (subpel_offset order k) of the grid best `centre`, scored by a
// group of kLanes adjacent lanes: sad(nxr, nyr) is this lane's share of the SAD at window position
// (nxr, nyr).  Returns the neighbour's key on every lane of the group, ~0 when it lies outside the
// window (uniform per group).
template <int kLanes, class Sad, class Key>
__device__ __forceinline__ unsigned long long me_neighbour(unsigned long long centre, int k, int side, Sad sad,
                                                           Key mkey) {
    const int cb0 = (int)(centre & 0xffff), bxr = cb0 % side, byr = cb0 / side;
    int ddx, ddy;
    subpel_offset(k, &ddx, &ddy);
    const int nxr = bxr + ddx, nyr = byr + ddy;
    const bool inside = nxr >= 0 && nxr < side && nyr >= 0 && nyr < side;
    int d = inside ? sad(nxr, nyr) : 0;
    for (int o = kLanes / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
    return inside ? mkey((uint32_t)d, nxr, nyr) : ~0ull;
}
// Half- then quarter-sample refinement of kN vectors (vx, vy, cost) at once, the whole workgroup
// calling.  The 8 candidates of a step around vector pi are scored by groups of 256 / (8 kN) lanes;
// this lane is lane `sub` of candidate k of vector pi and owns the 8 source samples at (xx, yy) of
// the macroblock (srcw).  sp[pi]: the footprint staged around the integer match (vx, vy)[pi] on entry.
// A step publishes its costs in cand (two barriers) and every thread takes the first lower cost in
// subpel_offset order.  on: false on a lane that owns no samples (an 8x8 quadrant fills 8 of the
// group's 16 lanes); its (xx, yy) still has to lie inside the macroblock.
template <int kN>
__device__ __forceinline__ void me_refine(const uint8_t (*sp)[4][18][kSpW], uint32_t (*cand)[8], const uint32_t* srcw,
                                          int pi, int k, int sub, int xx, int yy, int lambda, int* vx, int* vy,
                                          uint32_t* cost, bool on = true) {
    const uint32_t s0 = srcw[yy * 4 + (xx >> 2)], s1 = srcw[yy * 4 + (xx >> 2) + 1];
    const int base_x4 = xx * 4 + 4 - vx[pi], base_y4 = yy * 4 + 4 - vy[pi];  // local qpel coords = base + candidate mv
    for (int step = 2; step >= 1; step >>= 1) {
        int ddx, ddy;
        subpel_offset(k, &ddx, &ddy);
        const int cx = vx[pi] + ddx * step, cy = vy[pi] + ddy * step;
        int d = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            d += abs(byte_of(j < 4 ? s0 : s1, j & 3) - qpel_lds(sp[pi], base_x4 + 4 * j + cx, base_y4 + cy));
        }
        if (!on) d = 0;
        for (int o = kMeThreads / (16 * kN); o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
        __syncthreads();  // the previous step's readers are done with cand
        if (sub == 0) cand[pi][k] = me_cost((uint32_t)d, lambda, cx, cy);
        __syncthreads();
        for (int q = 0; q < kN; ++q) {
            int bdx = 0, bdy = 0;
            uint32_t bcost = cost[q];
            for (int kk = 0; kk < 8; ++kk) {
                const uint32_t cc = cand[q][kk];
                if (cc < bcost) {
                    int ex, ey;
                    subpel_offset(kk, &ex, &ey);
                    bcost = cc;
                    bdx = ex * step;
                    bdy = ey * step;
                }
            }
            vx[q] += bdx;
            vy[q] += bdy;
            cost[q] = bcost;
        }
    }
}
// Thread 0 stores the macroblock's motion in mbs[mbi]; every thread gets it back.  The vectors are
// local to the search centre (cx, cy; full samples), which is added here.  pvx / pvy: the two
// partition vectors of a 16x8 / 8x16 macroblock (a 16x16 one stores zeros).
__device__ __forceinline__ MbInfo store_motion(MbInfo* __restrict__ mbs, int mbi, int tid, int cx, int cy, int mvx,
                                               int mvy, int part, const int (&pvx)[2], const int (&pvy)[2]) {
    MbInfo out;
    out.mvx = (int16_t)(4 * cx + mvx);
    out.mvy = (int16_t)(4 * cy + mvy);
    out.part = (uint8_t)part;
    for (int i = 0; i < 2; ++i) {
        out.pmv[2 * i] = part == kPart16x16 ? 0 : (int16_t)(4 * cx + pvx[i]);
        out.pmv[2 * i + 1] = part == kPart16x16 ? 0 : (int16_t)(4 * cy + pvy[i]);
    }
    if (tid == 0) {
        MbInfo& m = mbs[mbi];
        m.mvx = out.mvx;
        m.mvy = out.mvy;
        m.part = out.part;
        for (int i = 0; i < 4; ++i) m.pmv[i] = out.pmv[i];
    }
    return out;
}
// The same for a 16x16 macroblock.
__device__ __forceinline__ MbInfo store_motion(MbInfo* __restrict__ mbs, int mbi, int tid, int cx, int cy, int mvx,
                                               int mvy) {
    const int none[2] = {0, 0};
    return store_motion(mbs, mbi, tid, cx, cy, mvx, mvy, kPart16x16, none, none);
}
// The same for a P_8x8 macroblock: the vectors of quadrants TL, TR, BL, BR (h264_gpu.h MbInfo).
__device__ __forceinline__ MbInfo store_motion_quads(MbInfo* __restrict__ mbs, int mbi, int tid, int cx, int cy,
                                                     const int (&qvx)[4], const int (&qvy)[4]) {
    MbInfo out;
    out.part = kPart8x8;
#pragma unroll
    for (int q = 0; q < 4; ++q) set_quad_mv(out, q, 4 * cx + qvx[q], 4 * cy + qvy[q]);
    if (tid == 0) {
        MbInfo& m = mbs[mbi];
        m.mvx = out.mvx;
        m.mvy = out.mvy;
        m.part = out.part;
        for (int i = 0; i < 4; ++i) m.pmv[i] = out.pmv[i];
        for (int i = 0; i < 2; ++i) m.pmv3[i] = out.pmv3[i];
    }
    return out;
}
// Returns the motion it stored in mbs[mbi] (mvx, mvy, part, pmv; the same on every thread): the
// fused kernel codes the macroblock from it without reading it back.  win_lds: kWinWords of LDS.
// kScroll (H.264 with EncoderConfig::scroll_range): a macroblock that fails the static exit looks at
// the picture's scroll hint g (h264_mb.h scroll_use) and takes vector 4g outright, or builds its
// window, candidates and footprints around the centre g instead of zero.  Vectors inside the body
// stay local to the centre -- so does the rate term of me_cost -- and the centre is added to what
// is stored.  Without kScroll the centre is the constant zero and the body is what it was.
// kQuad (H.264 with EncoderConfig::partitions 2; the state's partitions is then non-zero): every 8x8
// quadrant keeps a running best of its own beside the halves', and the macroblock becomes P_8x8 --
// four vectors, pmv3 stored and returned as well -- when that is strictly cheaper than the three
// other shapes (me_search_parts_cpu has the rules).  Without kQuad the body is what it was.
template <bool kScroll, bool kQuad = false>
__device__ __forceinline__ MbInfo me_full_body(const Geometry& g, const MeState& st, const uint8_t* __restrict__ src_y,
                                               MbInfo* __restrict__ mbs, uint32_t* win_lds,
                                               const int32_t* __restrict__ hint = nullptr) {
    static_assert(kMeThreads == 256, "the neighbour and refinement layouts: 8 candidates x 32 lanes");
    __shared__ uint8_t sp2[2][4][18][kSpW];   // sub-sample footprints: the 16x16 match, or two partitions
    __shared__ int16_t fp_b1[2][kFpRows][kSpW];
    __shared__ uint32_t srcw[64];
    __shared__ unsigned long long red[kMeWaves];
    __shared__ uint32_t cand_cost[8];
    __shared__ uint32_t s_sad0[4];

    const int mbi = blockIdx.x;  // default dispatch order (XCD mappings measured: profiles/r01_xcd)
    const int mbx = mbi % g.mb_w, mby = mbi / g.mb_w;
    const int x0 = mbx * 16, y0 = mby * 16;
    const int tid = threadIdx.x, lane = tid & 63;
    const int R = me_range(st.search_range);
    const int W = 16 + 2 * R;
    const uint8_t* __restrict__ ref = st.ref;
    const int lambda = lambda_sad(st.qp);

    // static-block early exit first: SAD of the zero vector from one source and one reference
    // pixel per thread (same rule as the CPU encoder), so the ~70 % static MBs of a desktop
    // never load the search window (a separate static pre-pass kernel feeding a list of the
    // moving MBs was measured slower: its atomic list append serialises, profiles/r02_me)
    constexpr int kWs4 = kWinStride / 4;
    int cx = 0, cy = 0;  // the centre of the search, full samples
    {
        if (tid < 64) {
            uint32_t sw;
            const uint32_t d = zero_sad_wave(src_y, ref, g.pitch, x0, y0, tid, &sw);
            if (tid == 0) s_sad0[0] = d;
        }
        __syncthreads();
        const uint32_t sad0 = s_sad0[0];
        if (sad0 <= static_sad(st.qp)) {  // uniform across the workgroup
            // written out: through store_motion the compiler merges this store with the search's last
            // one, and k_me_full and k_me_full_val need two more SGPRs (profiles/search_once)
            MbInfo out;
            out.mvx = out.mvy = 0;
            out.part = kPart16x16;
            out.pmv[0] = out.pmv[1] = out.pmv[2] = out.pmv[3] = 0;
            if (tid == 0) {
                MbInfo& m = mbs[mbi];
                m.mvx = 0;
                m.mvy = 0;
                m.part = kPart16x16;
                m.pmv[0] = m.pmv[1] = m.pmv[2] = m.pmv[3] = 0;
            }
            return out;
        }
        if constexpr (kScroll) {
            const int gx = hint[0], gy = hint[1];  // uniform (k_scroll_decide's, the kernel before)
            if (gx | gy) {
                if (tid < 64) {  // one wave: the 16x16 SAD at the integer vector g, edge-clamped
                    const int r = tid >> 2, c4 = (tid & 3) * 4;
                    const uint32_t sw = *reinterpret_cast<const uint32_t*>(src_y + (y0 + r) * g.pitch + x0 + c4);
                    uint32_t rw = 0;
                    for (int k = 0; k < 4; ++k)
                        rw |= (uint32_t)ref_px(ref, g.pitch, g.coded_w, g.coded_h, x0 + gx + c4 + k, y0 + gy + r) << (8 * k);
                    const int d = wave_sum((int)__builtin_amdgcn_sad_u8(sw, rw, 0u));
                    if (tid == 0) s_sad0[1] = (uint32_t)d;
                }
                __syncthreads();
                const int use = scroll_use(s_sad0[1], sad0, st.qp);
                if (use == kScrollExit) return store_motion(mbs, mbi, tid, gx, gy, 0, 0);  // uniform
                if (use == kScrollCentre) cx = gx, cy = gy;
            }
        }
    }
    // search window straight from the reference picture, edge-clamped.  Its left edge x0 - R - 4 is
    // a multiple of 4 and so is the coded width: a window dword lies wholly inside a picture row
    // (one dword load) or wholly beside it (the row's edge sample four times) -- no byte gathers.
    const int wrows = W + 2 * kWinPadY + 1, wx0 = x0 + cx - R - kWinPadX, wy0 = y0 + cy - R - kWinPadY;
    const bool dwords = (g.pitch & 3) == 0 && (reinterpret_cast<uintptr_t>(ref) & 3) == 0;
    for (int i = tid; i < wrows * kWs4; i += kMeThreads) {
        const int wy = i / kWs4, wx4 = (i - wy * kWs4) * 4;
        uint32_t w = 0u;
        if (wx4 < W + 2 * kWinPadX) {
            const int py = min(max(wy0 + wy, 0), g.coded_h - 1), px = wx0 + wx4;
            const uint8_t* row = ref + (size_t)py * g.pitch;
            if (kScroll && (wx0 & 3))  // a centre off the dword grid: a dword may straddle the picture's edge
                for (int k = 0; k < 4; ++k) w |= (uint32_t)row[min(max(px + k, 0), g.coded_w - 1)] << (8 * k);
            else if (px < 0)
                w = row[0] * 0x01010101u;
            else if (px >= g.coded_w)
                w = row[g.coded_w - 1] * 0x01010101u;
            else if (dwords)
                w = *reinterpret_cast<const uint32_t*>(row + px);
            else
                w = row[px] | ((uint32_t)row[px + 1] << 8) | ((uint32_t)row[px + 2] << 16) | ((uint32_t)row[px + 3] << 24);
        }
        win_lds[i] = w;
    }
    // the search addresses the window from its first candidate position (vector (-R, -R))
    const uint32_t* win32 = win_lds + kWinPadY * kWs4 + kWinPadX / 4;
    // window byte (in win_lds) one sample up-left of the integer match (vx, vy): build_footprints
    auto fp_org = [&](int vx, int vy) {
        return ((vy >> 2) + R + kWinPadY - 1) * kWinStride + (vx >> 2) + R + kWinPadX - 1;
    };
    if (tid < 64) {
        const int r = tid >> 2, c = (tid & 3) * 4;
        srcw[tid] = *reinterpret_cast<const uint32_t*>(src_y + (y0 + r) * g.pitch + x0 + c);
    }
    __syncthreads();

    // Each thread scores four horizontally adjacent candidates per step: their 16x16 blocks
    // share one dword-aligned 20-byte row span of the window, so every row costs 5 LDS reads
    // (instead of 5 per candidate) and 4 v_qsad_pk_u16_u8 (qsad4; 12 v_alignbyte + 16 v_sad_u8
    // before: k_p_fused 61.8 -> 55.3 us at 1080p, k_me_full 87.1 -> 78.9 us at 4K, profiles/p_quad).
    const int side = 2 * R + 1, gw = (side + 3) >> 2, ngroups = side * gw;
    unsigned long long best = ~0ull;
    const bool coarse = st.me_coarse != 0;
    // coarse mode (me_coarse): the even-offset grid first -- two candidates per thread (window
    // shifts 0 and 2 of a dword group), (R + 1) * gw tasks in one pass -- then the 8 integer
    // neighbours of its best (me_search_cpu does the same)
    const bool parts = st.partitions != 0;  // 16x8 / 8x16 partitionings searched too (me_search_parts_cpu)
    auto mkey = [&](uint32_t sad, int dxr, int dyr) {
        const int dx = dxr - R, dy = dyr - R;
        const uint32_t cost = me_cost(sad, lambda, 4 * dx, 4 * dy);
        const uint32_t dist = (uint32_t)(abs(dx) + abs(dy));
        return ((unsigned long long)cost << 32) | (dist << 16) | (uint32_t)(dyr * side + dxr);
    };
    // partitions: per candidate the SAD of each 8x8 quadrant (TL, TR, BL, BR); the 16x16 key is
    // their sum (so the 16x16 decision is unchanged) and shapes T / B / L / R keep their own best
    unsigned long long pb[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    unsigned long long qb[4] = {~0ull, ~0ull, ~0ull, ~0ull};  // kQuad: quadrants TL, TR, BL, BR
    auto visit_quads = [&](const uint32_t* qd, int dxr, int dyr) {
        if constexpr (kQuad)
            for (int i = 0; i < 4; ++i) qb[i] = kmin(qb[i], mkey(qd[i], dxr, dyr));
        best = kmin(best, mkey(qd[0] + qd[1] + qd[2] + qd[3], dxr, dyr));
        pb[0] = kmin(pb[0], mkey(qd[0] + qd[1], dxr, dyr));
        pb[1] = kmin(pb[1], mkey(qd[2] + qd[3], dxr, dyr));
        pb[2] = kmin(pb[2], mkey(qd[0] + qd[2], dxr, dyr));
        pb[3] = kmin(pb[3], mkey(qd[1] + qd[3], dxr, dyr));
    };
    if (parts) {
        // tasks: the even grid (coarse, shifts 0 and 2 of a dword group) or every group (shifts 0..3)
        const int nsh = coarse ? 2 : 4, ntp = coarse ? (R + 1) * gw : ngroups;
        for (int q = tid; q < ntp; q += kMeThreads) {
            const int dyr = coarse ? 2 * (q / gw) : q / gw, g = q % gw;
            // one packed accumulator per quadrant: the four shifted SADs of the dword group as 16-bit
            // sums (a quadrant's is <= 8 * 8 * 255), a v_qsad_pk_u16_u8 per source dword and row
            uint64_t acc[4] = {0, 0, 0, 0};
#pragma unroll
            for (int h = 0; h < 2; ++h)  // the top quadrants' rows, then the bottom ones'
#pragma unroll 2
                for (int r = 8 * h; r < 8 * h + 8; ++r)
                    me_row(win32, srcw, (dyr + r) * kWs4 + g, r, acc[2 * h], acc[2 * h + 1]);
#pragma unroll
            for (int si = 0; si < 4; ++si) {
                if (si >= nsh) break;
                const int dxr = 4 * g + (coarse ? 2 * si : si);
                if (dxr >= side) break;
                const int sh = 16 * (coarse ? 2 * si : si);
                const uint32_t qd[4] = {(uint32_t)(acc[0] >> sh) & 0xffffu, (uint32_t)(acc[1] >> sh) & 0xffffu,
                                        (uint32_t)(acc[2] >> sh) & 0xffffu, (uint32_t)(acc[3] >> sh) & 0xffffu};
                visit_quads(qd, dxr, dyr);
            }
        }
    } else {
        auto visit = [&](uint32_t sad, int dxr, int dyr) { best = kmin(best, mkey(sad, dxr, dyr)); };
        if (coarse)
            me_score16<true>(win32, srcw, (R + 1) * gw, gw, side, tid, visit);
        else
            me_score16<false>(win32, srcw, ngroups, gw, side, tid, visit);
    }
    best = wave_min_u64(best);
    if (lane == 0) red[tid >> 6] = best;
    __shared__ unsigned long long pred4[4][kMeWaves];  // partitions: [shape][wave]
    if (parts) {
#pragma unroll
        for (int sh = 0; sh < 4; ++sh) {
            const unsigned long long v = wave_min_u64(pb[sh]);
            if (lane == 0) pred4[sh][tid >> 6] = v;
        }
    }
    __shared__ unsigned long long qred4[kQuad ? 4 : 1][kMeWaves];  // kQuad: [quadrant][wave]
    if constexpr (kQuad) {
        if (parts) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned long long v = wave_min_u64(qb[i]);
                if (lane == 0) qred4[i][tid >> 6] = v;
            }
        }
    }
    __syncthreads();
    unsigned long long b = block_min(red);
    unsigned long long pbest[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    if (parts)
        for (int sh = 0; sh < 4; ++sh) pbest[sh] = block_min(pred4[sh]);
    unsigned long long qbest[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    if constexpr (kQuad) {
        if (parts)
            for (int i = 0; i < 4; ++i) qbest[i] = block_min(qred4[i]);
    }
    const uint8_t* wb = reinterpret_cast<const uint8_t*>(win32);
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(srcw);
    if (parts && coarse) {
        // the 8 integer neighbours of each partition's grid best: 32 (shape, neighbour) pairs of
        // 128-sample rectangles, 8 lanes (16 samples) each
        __shared__ unsigned long long pnkey[4][8];
        const int ev = tid >> 3, sub = tid & 7, sh = ev >> 3, k = ev & 7;
        const unsigned long long nk = me_neighbour<8>(pbest[sh], k, side, [&](int nxr, int nyr) {
            // T / B: one 16-sample row each (row sub of the half); L / R: two 8-sample rows
            int d = 0;
            for (int part_row = 0; part_row < 2; ++part_row) {
                const int rr = sh < 2 ? (sh == 0 ? sub : 8 + sub) : 2 * sub + part_row;
                const int c0 = sh < 2 ? 8 * part_row : (sh == 2 ? 0 : 8);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    d += abs((int)sb[rr * 16 + c0 + j] - (int)wb[(nyr + rr) * kWinStride + nxr + c0 + j]);
            }
            return d;
        }, mkey);
        if (sub == 0) pnkey[sh][k] = nk;
        __syncthreads();
        for (int s2 = 0; s2 < 4; ++s2)
            for (int i = 0; i < 8; ++i) pbest[s2] = kmin(pbest[s2], pnkey[s2][i]);
        if constexpr (kQuad) {
            // ... and of each quadrant's: 32 (quadrant, neighbour) pairs of 64-sample squares, a row
            // of 8 samples per lane
            __shared__ unsigned long long qnkey[4][8];
            const int qi = ev >> 3;
            const unsigned long long qk = me_neighbour<8>(qbest[qi], k, side, [&](int nxr, int nyr) {
                const int rr = 8 * (qi >> 1) + sub, c0 = 8 * (qi & 1);
                int d = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    d += abs((int)sb[rr * 16 + c0 + j] - (int)wb[(nyr + rr) * kWinStride + nxr + c0 + j]);
                return d;
            }, mkey);
            if (sub == 0) qnkey[qi][k] = qk;
            __syncthreads();
            for (int s2 = 0; s2 < 4; ++s2)
                for (int i = 0; i < 8; ++i) qbest[s2] = kmin(qbest[s2], qnkey[s2][i]);
        }
    }
    if (coarse) {  // the 8 integer neighbours of the grid best: one per 32-lane group, 8 samples per lane
        __shared__ unsigned long long nkey[8];
        const int k = tid >> 5, sub = tid & 31, py = sub >> 1, px0 = (sub & 1) * 8;
        const unsigned long long nk = me_neighbour<32>(b, k, side, [&](int nxr, int nyr) {
            const uint8_t* wrow = wb + (nyr + py) * kWinStride + nxr + px0;
            const uint32_t s0 = srcw[py * 4 + (px0 >> 2)], s1 = srcw[py * 4 + (px0 >> 2) + 1];
            int d = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) d += abs(byte_of(j < 4 ? s0 : s1, j & 3) - (int)wrow[j]);
            return d;
        }, mkey);
        if (sub == 0) nkey[k] = nk;
        __syncthreads();
        for (int i = 0; i < 8; ++i) b = kmin(b, nkey[i]);
    }
    const int cbest = (int)(b & 0xffff);
    int mvx = 4 * ((cbest % side) - R), mvy = 4 * ((cbest / side) - R);

    if (parts) {
        // shape decision on the integer costs: 16x16 unless a partitioning's two costs + 2 lambda
        // (mb_type bits) are lower, 16x8 before 8x16 on ties
        const uint32_t c16 = (uint32_t)(b >> 32);
        const uint32_t chz = (uint32_t)(pbest[0] >> 32) + (uint32_t)(pbest[1] >> 32) + 2u * (uint32_t)lambda;
        const uint32_t cvt = (uint32_t)(pbest[2] >> 32) + (uint32_t)(pbest[3] >> 32) + 2u * (uint32_t)lambda;
        const int part = (c16 <= chz && c16 <= cvt) ? kPart16x16 : (chz <= cvt ? kPart16x8 : kPart8x16);
        if constexpr (kQuad) {
            // P_8x8 only when strictly cheaper than all three: four costs + 8 lambda (mb_type ue(3)
            // and four sub_mb_type ue(0), 9 bits against the 1 of 16x16 -- the "+ 2 lambda" accounting)
            const uint32_t c8 = (uint32_t)(qbest[0] >> 32) + (uint32_t)(qbest[1] >> 32) + (uint32_t)(qbest[2] >> 32) +
                                (uint32_t)(qbest[3] >> 32) + 8u * (uint32_t)lambda;
            if (c8 < c16 && c8 < chz && c8 < cvt) {  // uniform
                int qvx[4], qvy[4];
                uint32_t qcost[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int cb = (int)(qbest[i] & 0xffff);
                    qvx[i] = 4 * ((cb % side) - R);
                    qvy[i] = 4 * ((cb / side) - R);
                    qcost[i] = (uint32_t)(qbest[i] >> 32);
                }
                if (st.subpel) {
                    // per quadrant over its own square, quadrants {0, 1} then {2, 3} through the two
                    // footprints: 16 lanes per candidate as for the halves, 8 of them hold a row
                    __shared__ uint32_t qcand[2][8];
                    const int pi = tid >> 7, k = (tid >> 4) & 7, sub = tid & 15;
#pragma unroll
                    for (int pass = 0; pass < 2; ++pass) {
                        build_footprints(reinterpret_cast<const uint8_t*>(win_lds), fp_org(qvx[2 * pass], qvy[2 * pass]),
                                         fp_org(qvx[2 * pass + 1], qvy[2 * pass + 1]), 2, sp2, fp_b1, tid);
                        __syncthreads();
                        me_refine<2>(sp2, qcand, srcw, pi, k, sub, 8 * pi, 8 * pass + (sub & 7), lambda, qvx + 2 * pass,
                                     qvy + 2 * pass, qcost + 2 * pass, sub < 8);
                    }
                }
                return store_motion_quads(mbs, mbi, tid, cx, cy, qvx, qvy);
            }
        }
        if (part != kPart16x16) {
            const int s0 = part == kPart16x8 ? 0 : 2;  // pbest index of partition 0
            int pvx[2], pvy[2];
            uint32_t pcost[2];
            for (int i = 0; i < 2; ++i) {
                const int cb = (int)(pbest[s0 + i] & 0xffff);
                pvx[i] = 4 * ((cb % side) - R);
                pvy[i] = 4 * ((cb / side) - R);
                pcost[i] = (uint32_t)(pbest[s0 + i] >> 32);
            }
            if (st.subpel) {
                // half then quarter pel per partition over its own rectangle: an 18x18 footprint
                // per partition, 16 lanes (8 samples each) per candidate, both partitions at once
                __shared__ uint32_t pcand[2][8];
                build_footprints(reinterpret_cast<const uint8_t*>(win_lds), fp_org(pvx[0], pvy[0]),
                                 fp_org(pvx[1], pvy[1]), 2, sp2, fp_b1, tid);
                __syncthreads();
                const int pi = tid >> 7, k = (tid >> 4) & 7, sub = tid & 15;
                // the 8 samples of this lane inside the partition rectangle
                const int rx = part == kPart8x16 ? 8 * pi : 0, ry = part == kPart16x8 ? 8 * pi : 0;
                const int prow = part == kPart16x8 ? (sub >> 1) : sub, pcol = part == kPart16x8 ? (sub & 1) * 8 : 0;
                me_refine<2>(sp2, pcand, srcw, pi, k, sub, rx + pcol, ry + prow, lambda, pvx, pvy, pcost);
            }
            // mvx, mvy: the integer 16x16 vector (unused by the partitioned MB)
            return store_motion(mbs, mbi, tid, cx, cy, mvx, mvy, part, pvx, pvy);  // uniform
        }
    }

    if (st.subpel) {
        // half-pel then quarter-pel around the integer match.  Every candidate of both steps
        // lies in one 18x18 footprint of the F/H/V/J samples (the integer match +-1 sample),
        // interpolated once from the staged window; the 8 neighbours of a step are
        // scored at once, one per 32-lane half-wave group (8 pixels per lane, source from
        // srcw), a 5-step xor shuffle reduces each group, one barrier publishes the costs.
        build_footprints(reinterpret_cast<const uint8_t*>(win_lds), fp_org(mvx, mvy), 0, 1, sp2, fp_b1, tid);
        __syncthreads();
        uint32_t cur_cost = (uint32_t)(b >> 32);
        const int k = tid >> 5, sub = tid & 31;
        me_refine<1>(sp2, &cand_cost, srcw, 0, k, sub, (sub & 1) * 8, sub >> 1, lambda, &mvx, &mvy, &cur_cost);
    }
    return store_motion(mbs, mbi, tid, cx, cy, mvx, mvy);
}

// The search is the first kernel of an H.264 P picture: it publishes the frame state for the later
// kernels and stamps the start (StateArg), or reads the published copy (hipGraph, HEVC, VP8).
// k_me_full_val is the launch on the side stream beside the previous picture's in-loop filter:
// the same body, always with the state by value (a name of its own in kernel traces).
__global__ __launch_bounds__(kMeThreads) void k_me_full(Geometry g, StateArg sa, const uint8_t* __restrict__ src_y,
                                                        MbInfo* __restrict__ mbs) {
    __shared__ uint32_t win_lds[kWinWords];
    publish_state(sa);
    me_full_body<false>(g, sa.publish ? me_state(sa.v) : me_state(*sa.dst), src_y, mbs, win_lds);
}
__global__ __launch_bounds__(kMeThreads) void k_me_full_val(Geometry g, StateArg sa, const uint8_t* __restrict__ src_y,
                                                            MbInfo* __restrict__ mbs) {
    __shared__ uint32_t win_lds[kWinWords];
    publish_state(sa);
    me_full_body<false>(g, me_state(sa.v), src_y, mbs, win_lds);
}
// The same two with the scroll hint (H.264 pictures after k_scroll_probe, which stamped the start)
__global__ __launch_bounds__(kMeThreads) void k_me_full_scroll(Geometry g, StateArg sa,
                                                               const uint8_t* __restrict__ src_y,
                                                               MbInfo* __restrict__ mbs,
                                                               const int32_t* __restrict__ hint) {
    __shared__ uint32_t win_lds[kWinWords];
    publish_state(sa);
    me_full_body<true>(g, sa.publish ? me_state(sa.v) : me_state(*sa.dst), src_y, mbs, win_lds, hint);
}
__global__ __launch_bounds__(kMeThreads) void k_me_full_val_scroll(Geometry g, StateArg sa,
                                                                   const uint8_t* __restrict__ src_y,
                                                                   MbInfo* __restrict__ mbs,
                                                                   const int32_t* __restrict__ hint) {
    __shared__ uint32_t win_lds[kWinWords];
    publish_state(sa);
    me_full_body<true>(g, me_state(sa.v), src_y, mbs, win_lds, hint);
}
// The four again with the 8x8 quadrants searched (EncoderConfig::partitions 2): kernels of their own,
// so that the ones above keep their registers and occupancy (profiles/p8x8/NOTES.md).  Entry points
// written out like the four above: one shared templated entry point changed the instructions of
// k_me_full and k_me_full_scroll.
__global__ __launch_bounds__(kMeThreads) void k_me_full_q8(Geometry g, StateArg sa, const uint8_t* __restrict__ src_y,
                                                           MbInfo* __restrict__ mbs) {
    __shared__ uint32_t win_lds[kWinWords];
    publish_state(sa);
    me_full_body<false, true>(g, sa.publish ? me_state(sa.v) : me_state(*sa.dst), src_y, mbs, win_lds);
}
__global__ __launch_bounds__(kMeThreads) void k_me_full_val_q8(Geometry g, StateArg sa,
                                                               const uint8_t* __restrict__ src_y,
                                                               MbInfo* __restrict__ mbs) {
    __shared__ uint32_t win_lds[kWinWords];
    publish_state(sa);
    me_full_body<false, true>(g, me_state(sa.v), src_y, mbs, win_lds);
}
__global__ __launch_bounds__(kMeThreads) void k_me_full_scroll_q8(Geometry g, StateArg sa,
                                                                  const uint8_t* __restrict__ src_y,
                                                                  MbInfo* __restrict__ mbs,
                                                                  const int32_t* __restrict__ hint) {
    __shared__ uint32_t win_lds[kWinWords];
    publish_state(sa);
    me_full_body<true, true>(g, sa.publish ? me_state(sa.v) : me_state(*sa.dst), src_y, mbs, win_lds, hint);
}
__global__ __launch_bounds__(kMeThreads) void k_me_full_val_scroll_q8(Geometry g, StateArg sa,
                                                                      const uint8_t* __restrict__ src_y,
                                                                      MbInfo* __restrict__ mbs,
                                                                      const int32_t* __restrict__ hint) {
    __shared__ uint32_t win_lds[kWinWords];
    publish_state(sa);
    me_full_body<true, true>(g, me_state(sa.v), src_y, mbs, win_lds, hint);
}

// ------------------------------------------------------------------ scroll probe
// One 256-thread workgroup per probe macroblock of the lattice (h264_mb.h scroll_is_probe), before
// the search of a P picture with EncoderConfig::scroll_range.  A probe whose zero vector passes the
// static exit does nothing.  Every other one stages two edge-clamped strips of the reference in
// LDS -- 16 wide x (16 + 2D) tall and (16 + 2D) wide x 16 tall, whole dwords as the search window --
// and scores the 16x16 SAD of every (0, d) and (d, 0), 0 < |d| <= D: the vertical candidates one
// per thread (v_sad_u8 on the four dwords of a row), the horizontal ones four per v_qsad_pk_u16_u8
// as the search does, a thread per dword group and half of the rows.  The best candidate by
// scroll_probe_key votes for its bin when it is a static match (integer atomics: the histogram
// does not depend on the order).  k_scroll_decide, one workgroup after it, takes the decision
// (scroll_bin_key, scroll_decide), stores the hint and leaves the histogram zero for the slot's next
// picture.  (The decision in the probe's last workgroup, behind a counter as k_pack's, needs the
// votes ordered before the count -- a release per workgroup: it added 55 us to a still 1080p
// picture, where every probe leaves at once, against 21 us for the two kernels (13 + 5 us of
// kernel time): profiles/scroll_hint/NOTES.md.)
constexpr int kProbeThreads = 256, kProbeWaves = kProbeThreads / 64;
constexpr int kStripVWords = (16 + 2 * kScrollMaxReach) * 4;
constexpr int kStripHS4 = kScrollMaxReach / 2 + 5;  // dwords per row of the horizontal strip: 16 + 2D bytes + a group's over-read
constexpr int kStripHWords = 16 * kStripHS4;
__global__ __launch_bounds__(kProbeThreads) void k_scroll_probe(Geometry g, StateArg sa,
                                                                const uint8_t* __restrict__ src_y,
                                                                uint32_t* __restrict__ hist, int D) {
    __shared__ uint32_t vs[kStripVWords];
    __shared__ uint32_t hs[kStripHWords];
    __shared__ uint32_t srcw[64];
    __shared__ unsigned long long red[kProbeWaves];
    __shared__ uint32_t s_flag[1];
    publish_state(sa);
    const FrameState& f = state_of(sa);
    const uint8_t* __restrict__ ref = f.me_ref ? f.me_ref : f.ref_y;
    const int qp = f.qp;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int npx = scroll_probes_x(g.mb_w);
    const int x0 = (int)(blockIdx.x % npx) * kScrollLattice * 16, y0 = (int)(blockIdx.x / npx) * kScrollLattice * 16;
    if (tid < 64) {  // the static exit of the search
        uint32_t sw;
        const uint32_t d = zero_sad_wave(src_y, ref, g.pitch, x0, y0, tid, &sw);
        srcw[tid] = sw;
        if (tid == 0) s_flag[0] = d;
    }
    __syncthreads();
    if (s_flag[0] > static_sad(qp)) {  // uniform across the workgroup
        const bool dwords = (g.pitch & 3) == 0 && (reinterpret_cast<uintptr_t>(ref) & 3) == 0;
        for (int i = tid; i < (16 + 2 * D) * 4; i += kProbeThreads) {  // x0 .. x0 + 15 lies inside the picture
            const int wy = i >> 2, q = i & 3;
            const uint8_t* p = ref + (size_t)min(max(y0 - D + wy, 0), g.coded_h - 1) * g.pitch + x0 + 4 * q;
            vs[i] = dwords ? *reinterpret_cast<const uint32_t*>(p)
                           : (p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
        }
        // x0 - D and the coded width are multiples of 4: a dword lies wholly inside a row or beside it
        const int hw4 = D / 2 + 5;
        for (int i = tid; i < 16 * hw4; i += kProbeThreads) {
            const int r = i / hw4, wx4 = i - r * hw4, px = x0 - D + 4 * wx4;
            const uint8_t* row = ref + (size_t)(y0 + r) * g.pitch;
            uint32_t w;
            if (px < 0)
                w = row[0] * 0x01010101u;
            else if (px >= g.coded_w)
                w = row[g.coded_w - 1] * 0x01010101u;
            else if (dwords)
                w = *reinterpret_cast<const uint32_t*>(row + px);
            else
                w = row[px] | ((uint32_t)row[px + 1] << 8) | ((uint32_t)row[px + 2] << 16) | ((uint32_t)row[px + 3] << 24);
            hs[r * kStripHS4 + wx4] = w;
        }
        __syncthreads();
        unsigned long long best = ~0ull;
        for (int c = tid; c <= 2 * D; c += kProbeThreads) {  // vertical: (0, c - D)
            if (c == D) continue;
            uint32_t sad = 0;
#pragma unroll 4
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int q = 0; q < 4; ++q) sad = __builtin_amdgcn_sad_u8(srcw[r * 4 + q], vs[(c + r) * 4 + q], sad);
            const unsigned long long key = scroll_probe_key(sad, 0, c - D, D);
            best = key < best ? key : best;
        }
        {  // horizontal: thread 2 * grp + half scores rows 8 * half .. + 7 of candidates (4 grp + 0..3 - D, 0)
            const int grp = tid >> 1, half = tid & 1;
            const bool on = grp <= D / 2;
            uint64_t acc = 0;  // four shifted SADs, 16 bits each (a 16x16 SAD is <= 65,280)
            if (on) {
#pragma unroll 2
                for (int r = 8 * half; r < 8 * half + 8; ++r) {
                    const int a = r * kStripHS4 + grp;
                    const uint32_t w0 = hs[a], w1 = hs[a + 1], w2 = hs[a + 2], w3 = hs[a + 3], w4 = hs[a + 4];
                    acc = qsad4(w1, w0, srcw[r * 4 + 0], acc);
                    acc = qsad4(w2, w1, srcw[r * 4 + 1], acc);
                    acc = qsad4(w3, w2, srcw[r * 4 + 2], acc);
                    acc = qsad4(w4, w3, srcw[r * 4 + 3], acc);
                }
            }
            acc += __shfl_xor(acc, 1, 64);  // both halves: no field overflows into the next
            if (on && half == 0) {
#pragma unroll
                for (int sh = 0; sh < 4; ++sh) {
                    const int c = 4 * grp + sh;
                    if (c > 2 * D || c == D) continue;
                    const unsigned long long key = scroll_probe_key((uint32_t)(acc >> (16 * sh)) & 0xffffu, 1, c - D, D);
                    best = key < best ? key : best;
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o, 64);
            best = other < best ? other : best;
        }
        if (lane == 0) red[wave] = best;
        __syncthreads();
        if (tid == 0) {
            for (int i = 1; i < kProbeWaves; ++i) best = red[i] < best ? red[i] : best;
            if (scroll_key_votes(best, qp))
                __hip_atomic_fetch_add(&hist[scroll_key_bin(best)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
__global__ __launch_bounds__(kProbeThreads) void k_scroll_decide(int D, uint32_t* __restrict__ hist,
                                                                 int32_t* __restrict__ hint) {
    __shared__ unsigned long long red[kProbeWaves];
    __shared__ uint32_t tot[kProbeWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nbins = scroll_bins(D);
    unsigned long long win = 0;
    uint32_t total = 0;
    for (int b = tid; b < nbins; b += kProbeThreads) {
        const uint32_t v = hist[b];
        if (v) hist[b] = 0u;
        const unsigned long long key = scroll_bin_key(v, b, D);
        win = key > win ? key : win;
        total += v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(win, o, 64);
        win = other > win ? other : win;
        total += __shfl_xor(total, o, 64);
    }
    if (lane == 0) {
        red[wave] = win;
        tot[wave] = total;
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < kProbeWaves; ++i) {
            win = red[i] > win ? red[i] : win;
            total += tot[i];
        }
        int gx, gy;
        scroll_decide(win, total, D, &gx, &gy);
        hint[0] = gx;
        hint[1] = gy;
    }
}

// ------------------------------------------------------------------ inter encode
// One MB per wave, 4x4 blocks in "row" layout: lane 4b + r holds row r of block b (luma: all
// 64 lanes = 16 blocks; chroma: lanes 0..31 = 8 blocks).  Both 1-D passes of every transform
// run in-lane on a row, the column pass gathers the block's four rows with DPP quad
// broadcasts (no LDS round trips); the integer arithmetic is exactly fdct4x4 / idct4x4 /
// hadamard4x4 / quant4x4 / dequant4x4 (rows first, then columns), so the bitstream is
// unchanged.  A block-per-lane layout left 40 of 64 lanes idle in the transform phase.
// forward core transform of row r of a block whose rows sit in the quad: y = row r of Cf X Cf^T
__device__ __forceinline__ void fdct_row(const int* x, int r, int* y) {
    const int s03 = x[0] + x[3], d03 = x[0] - x[3], s12 = x[1] + x[2], d12 = x[1] - x[2];
    const int t[4] = {s03 + s12, 2 * d03 + d12, s03 - s12, d03 - 2 * d12};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int a0 = qbc<0>(t[c]), a1 = qbc<1>(t[c]), a2 = qbc<2>(t[c]), a3 = qbc<3>(t[c]);
        const int u03 = a0 + a3, e03 = a0 - a3, u12 = a1 + a2, e12 = a1 - a2;
        y[c] = r == 0 ? u03 + u12 : r == 1 ? 2 * e03 + e12 : r == 2 ? u03 - u12 : e03 - 2 * e12;
    }
}
// inverse core transform: residual row r from dequantised row d
__device__ __forceinline__ void idct_row(const int* d, int r, int* out) {
    const int e0 = d[0] + d[2], e1 = d[0] - d[2], e2 = (d[1] >> 1) - d[3], e3 = d[1] + (d[3] >> 1);
    const int f[4] = {e0 + e3, e1 + e2, e1 - e2, e0 - e3};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int b0 = qbc<0>(f[c]), b1 = qbc<1>(f[c]), b2 = qbc<2>(f[c]), b3 = qbc<3>(f[c]);
        const int g0 = b0 + b2, g1 = b0 - b2, g2 = (b1 >> 1) - b3, g3 = b1 + (b3 >> 1);
        const int v = r == 0 ? g0 + g3 : r == 1 ? g1 + g2 : r == 2 ? g1 - g2 : g0 - g3;
        out[c] = (v + 32) >> 6;
    }
}
// sum |Hadamard coefficients| of row r (satd4x4 before its halving)
__device__ __forceinline__ int had_row_abs(const int* x, int r) {
    const int t[4] = {x[0] + x[1] + x[2] + x[3], x[0] + x[1] - x[2] - x[3], x[0] - x[1] - x[2] + x[3],
                      x[0] - x[1] + x[2] - x[3]};
    int s = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int a = qbc<0>(t[c]), b = qbc<1>(t[c]), cc = qbc<2>(t[c]), d = qbc<3>(t[c]);
        const int v = r == 0 ? a + b + cc + d : r == 1 ? a + b - cc - d : r == 2 ? a - b - cc + d : a - b + cc - d;
        s += v < 0 ? -v : v;
    }
    return s;
}
// quant4x4 / dequant4x4 on row r (start = 1: the DC position is skipped)
__device__ __forceinline__ int quant_row(const int* y, int r, int qp, bool intra, int start, int* z) {
    const int qm = qp % 6, qbits = 15 + qp / 6;
    const int f = intra ? ((1 << qbits) / 3) : ((1 << qbits) / 6);
    int nz = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int i = r * 4 + c;
        if (i < start) {
            z[c] = 0;
            continue;
        }
        const int a = y[c] < 0 ? -y[c] : y[c];
        int q = (int)(((int64_t)a * kQuantMF[qm][kPosClass[i]] + f) >> qbits);
        q = q > kMaxLevel ? kMaxLevel : q;
        z[c] = y[c] < 0 ? -q : q;
        nz += (q != 0);
    }
    return nz;
}
__device__ __forceinline__ void dequant_row(const int* z, int r, int qp, int* d) {
    const int qm = qp % 6, qs = qp / 6;
#pragma unroll
    for (int c = 0; c < 4; ++c) d[c] = z[c] * kDequantV[qm][kPosClass[r * 4 + c]] * (1 << qs);
}

// Quarter-sample luma prediction of one macroblock straight from the reference picture (8.4.2.2.1;
// sample for sample luma_qpel() of the CPU encoder), by one wave.  The macroblock has n = 1 or 2
// vectors (partitions); (xa, ya) and (xb, yb) are the quarter-sample positions its top-left sample
// is predicted from under each.  The wave stages, per vector, the edge-clamped (16+5) x (16+5)
// sample window of the whole block -- reference sample (bx - 2 + c, by - 2 + r) at byte c of row r,
// rows of kMcStride bytes -- in LDS, both windows in one round of loads; then every lane
// interpolates its four samples (c0 .. c0+3, r), c0 a multiple of 4, under vector lpi from the
// 6 x 9 samples around them, into one dword (*out, first sample in the low byte).
constexpr int kMcStride = 24, kMcRows = 16 + 5, kMcWords = kMcRows * kMcStride / 4;
__device__ __forceinline__ void mc_luma_wave(uint32_t* __restrict__ w, const uint8_t* __restrict__ ref, int pitch,
                                             int cw, int ch, int n, int xa, int ya, int xb, int yb, int lane, int lpi,
                                             uint32_t* out) {
    const bool aligned = (pitch & 3) == 0 && (reinterpret_cast<uintptr_t>(ref) & 3) == 0;
    for (int i = lane; i < n * kMcWords; i += 64) {
        const int pi = i >= kMcWords ? 1 : 0, j = i - pi * kMcWords;
        const int wr = j / (kMcStride / 4), q = j - wr * (kMcStride / 4);
        const int xs = ((pi ? xb : xa) >> 2) - 2, ys = ((pi ? yb : ya) >> 2) - 2;
        uint32_t v;
        // rows wholly inside the picture's columns: a window dword from two aligned dwords of the row
        if (aligned && xs >= 0 && (xs & ~3) + kMcStride + 4 <= cw) {
            const int py = min(max(ys + wr, 0), ch - 1), px = xs + 4 * q;
            const uint32_t* qa = reinterpret_cast<const uint32_t*>(ref + (size_t)py * pitch + (px & ~3));
            const uint32_t sh = (uint32_t)(px & 3);
            v = sh ? __builtin_amdgcn_alignbyte(qa[1], qa[0], sh) : qa[0];
        } else {
            v = 0;
            for (int k = 0; k < 4; ++k) v |= (uint32_t)ref_px(ref, pitch, cw, ch, xs + 4 * q + k, ys + wr) << (8 * k);
        }
        w[i] = v;
    }
    wave_lds_sync();
    {
        const int xf = (lpi ? xb : xa) & 3, yf = (lpi ? yb : ya) & 3;
        w += lpi * kMcWords;
        const int r = lane >> 2, q0 = lane & 3;
        // window rows r .. r+5, bytes c0 .. c0+8 as three dwords a row; after every sample the rows
        // move one byte down, so the current sample is always s(2, 2) and the loop stays rolled
        // (18 live registers and one copy of the code, not 54 and four)
        uint32_t wd[6][3];
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) {
            const uint32_t* row = w + (r + rr) * (kMcStride / 4) + q0;
            wd[rr][0] = row[0];
            wd[rr][1] = row[1];
            wd[rr][2] = row[2];
        }
        auto s = [&](int rr, int c) { return byte_of(wd[rr][c >> 2], c & 3); };
        auto b1 = [&](int rr) { return tap6(s(rr, 0), s(rr, 1), s(rr, 2), s(rr, 3), s(rr, 4), s(rr, 5)); };
        auto v1 = [&](int c) { return tap6(s(0, c), s(1, c), s(2, c), s(3, c), s(4, c), s(5, c)); };
        auto b_at = [&](int rr) { return clip255((b1(rr) + 16) >> 5); };  // b at (x+1/2, row)
        auto h_at = [&](int c) { return clip255((v1(c) + 16) >> 5); };    // h at (column, y+1/2)
        auto j_val = [&]() { return clip255((tap6(b1(0), b1(1), b1(2), b1(3), b1(4), b1(5)) + 512) >> 10); };
        uint32_t packed = 0;
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            const int G = s(2, 2);
            int p;
            if ((xf | yf) == 0)
                p = G;
            else if (yf == 0)
                p = xf == 2 ? b_at(2) : ((xf == 1 ? G : s(2, 3)) + b_at(2) + 1) >> 1;
            else if (xf == 0)
                p = yf == 2 ? h_at(2) : ((yf == 1 ? G : s(3, 2)) + h_at(2) + 1) >> 1;
            else if (xf == 2 && yf == 2)
                p = j_val();
            else if (xf == 2)
                p = ((yf == 1 ? b_at(2) : b_at(3)) + j_val() + 1) >> 1;
            else if (yf == 2)
                p = ((xf == 1 ? h_at(2) : h_at(3)) + j_val() + 1) >> 1;
            else
                p = ((yf == 1 ? b_at(2) : b_at(3)) + (xf == 1 ? h_at(2) : h_at(3)) + 1) >> 1;
            packed |= (uint32_t)p << (8 * k);
#pragma unroll
            for (int rr = 0; rr < 6; ++rr) {
                wd[rr][0] = __builtin_amdgcn_alignbyte(wd[rr][1], wd[rr][0], 1);
                wd[rr][1] = __builtin_amdgcn_alignbyte(wd[rr][2], wd[rr][1], 1);
                wd[rr][2] >>= 8;
            }
        }
        *out = packed;
    }
}

// Test hook: one block by mc_luma_wave.
__global__ __launch_bounds__(64) void k_mc_luma_test(Geometry g, const uint8_t* __restrict__ ref, int x4, int y4,
                                                     uint8_t* __restrict__ out) {
    __shared__ uint32_t w[kMcWords];
    const int lane = threadIdx.x;
    uint32_t p = 0;
    mc_luma_wave(w, ref, g.pitch, g.coded_w, g.coded_h, 1, x4, y4, x4, y4, lane, 0, &p);
    reinterpret_cast<uint32_t*>(out)[lane] = p;  // lane = 4 * row + dword of the row
}

// What the coder reads of the frame state, taken once into scalar registers (as MeState).
struct CodeState {
    const uint8_t* ref_y;
    const uint8_t* ref_uv;
    uint8_t* rec_y;
    uint8_t* rec_uv;
    const uint8_t* prev_src;
    uint8_t* save_src;
    int qp, aq, intra_in_p, chroma_qp_offset;
};
__device__ __forceinline__ CodeState code_state(const FrameState& f) {
    return CodeState{f.ref_y, f.ref_uv, f.rec_y, f.rec_uv, f.prev_src, f.save_src, f.qp, f.aq, f.intra_in_p,
                     f.chroma_qp_offset};
}
// LDS of one coding wave
struct InterLds {
    __attribute__((aligned(4))) uint8_t pred[384];
    int16_t res[384];
    uint32_t mcw[2 * kMcWords];  // the windows of fractional vectors' prediction
    int cdc[8];
    int cdc_nz[2];
};
// One P macroblock coded by one wave (whole wave active): prediction under the motion `mi`
// (mvx / mvy / part / pmv), residual, transforms or their shortcuts, reconstruction, the rest of
// MbInfo and the macroblock's distortion (mb_sse[c * nmb + mbi], c = Y, U, V: k_scan_rows sums
// them).  L is the wave's own; it synchronises with wave_lds_sync() only.
// kQuad: the macroblock may be P_8x8 (part 3, four vectors: pmv3 is read too).  Without it part is
// at most 2 and the vector lookups leave the quadrant case out: the coder is then what it was.
template <bool kQuad = false>
__device__ __forceinline__ void inter_code_mb(const Geometry& g, const CodeState& fs, const uint8_t* __restrict__ src_y,
                                              const uint8_t* __restrict__ src_uv, MbInfo* __restrict__ mbs,
                                              int16_t* __restrict__ coef, uint32_t* __restrict__ mb_sse, int mbi,
                                              int lane, const MbInfo& motion, InterLds& L) {
    // the motion is the same on every lane: kept in scalar registers
    MbInfo mi;
    mi.mvx = (int16_t)__builtin_amdgcn_readfirstlane((int)motion.mvx);
    mi.mvy = (int16_t)__builtin_amdgcn_readfirstlane((int)motion.mvy);
    mi.part = (uint8_t)__builtin_amdgcn_readfirstlane((int)motion.part);
    for (int i = 0; i < 4; ++i) mi.pmv[i] = (int16_t)__builtin_amdgcn_readfirstlane((int)motion.pmv[i]);
    if constexpr (kQuad) {
        for (int i = 0; i < 2; ++i)
            mi.pmv3[i] = mi.part == kPart8x8 ? (int16_t)__builtin_amdgcn_readfirstlane((int)motion.pmv3[i]) : (int16_t)0;
    }
    const int nmb = g.mb_w * g.mb_h;
    const int mbx = mbi % g.mb_w, mby = mbi / g.mb_w;
    const int x0 = mbx * 16, y0 = mby * 16;
    const uint8_t* __restrict__ ref_y = fs.ref_y;
    const bool ref_dwords = (g.pitch & 3) == 0 && (reinterpret_cast<uintptr_t>(ref_y) & 3) == 0;
    const uint8_t* ref_uv = fs.ref_uv;
    const int cw = g.coded_w / 2, ch = g.coded_h / 2;
    int mvx = 0, mvy = 0;
    int lsad = 0;  // this lane's share of sum |luma residual| (adaptive quantisation)
    int tsad = 0;  // this lane's share of sum |src - previous src| (temporal class, aq 3)
    // "load" layout: lane 4 * r + q holds samples 4q .. 4q+3 of luma row r (source sw, prediction pw)
    // and chroma sample (lane & 7, lane >> 3) of both planes (prediction cpv, residual crs)
    uint32_t sw = 0, pw = 0;
    int cpv[2] = {0, 0}, crs[2] = {0, 0};
    {
        const int r = lane >> 2, c0 = (lane & 3) * 4;
        const Mv lv = px_mv<kQuad>(mi, c0, r);  // the lane's 4 luma samples lie in one partition
        mvx = lv.x;
        mvy = lv.y;
        sw = *reinterpret_cast<const uint32_t*>(src_y + (y0 + r) * g.pitch + x0 + c0);
        if (fs.aq >= 3) {
            // temporal class (h264_mb.h temporal_class): the source against the previous source,
            // displaced by the vector's integer part; this MB's source becomes the next frame's
            const int ix = mvx >> 2, iy = mvy >> 2;
            const int px = x0 + c0 + ix, py = y0 + r + iy;
            // inside the picture (no clamping): the 4 samples from one aligned dword, or two when
            // unaligned and the second stays inside the row's pitch
            if (px >= 0 && px + 4 <= g.coded_w && py >= 0 && py < g.coded_h &&
                ((px & 3) == 0 || (px & ~3) + 8 <= g.pitch)) {
                const uint32_t* qa = reinterpret_cast<const uint32_t*>(fs.prev_src + (size_t)py * g.pitch + (px & ~3));
                const uint32_t sh = (uint32_t)(px & 3);
                const uint32_t qw = sh ? __builtin_amdgcn_alignbyte(qa[1], qa[0], sh) : qa[0];
                tsad = (int)__builtin_amdgcn_sad_u8(sw, qw, 0u);
            } else {
                for (int k = 0; k < 4; ++k)
                    tsad += abs((int)((sw >> (8 * k)) & 0xff) -
                                ref_px(fs.prev_src, g.pitch, g.coded_w, g.coded_h, x0 + c0 + k + ix, y0 + r + iy));
            }
            *reinterpret_cast<uint32_t*>(fs.save_src + (y0 + r) * g.pitch + x0 + c0) = sw;
        }
        // luma prediction from the reference picture; the macroblock's one or two vectors are
        // uniform across the wave (the lane's 4 samples lie in partition lpi: vector (mvx, mvy))
        const int part = __builtin_amdgcn_readfirstlane((int)mi.part);
        const Mv va = blk_mv<kQuad>(mi, 0, 0), vb = blk_mv<kQuad>(mi, part == kPart8x16 ? 2 : 0, part == kPart16x8 ? 2 : 0);
        const int vax = __builtin_amdgcn_readfirstlane(va.x), vay = __builtin_amdgcn_readfirstlane(va.y);
        const int vbx = __builtin_amdgcn_readfirstlane(vb.x), vby = __builtin_amdgcn_readfirstlane(vb.y);
        bool quad_mc = false;
        if constexpr (kQuad) {
            if (part == kPart8x8) {
                // four vectors, some fractional: the two-window staging twice, quadrants {0, 1} then
                // {2, 3}; a lane's samples lie in quadrant 2 * (r >> 3) + (c0 >> 3).  All full-sample:
                // the lane's own vector below, as for the other shapes (va = vb = quadrant 0's there).
                int qx[4], qy[4], any = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const Mv v = quad_mv(mi, q);
                    qx[q] = v.x;  // mi is wave-uniform already
                    qy[q] = v.y;
                    any |= qx[q] | qy[q];
                }
                if (any & 3) {
                    uint32_t ptop = 0, pbot = 0;
                    mc_luma_wave(L.mcw, ref_y, g.pitch, g.coded_w, g.coded_h, 2, x0 * 4 + qx[0], y0 * 4 + qy[0],
                                 x0 * 4 + qx[1], y0 * 4 + qy[1], lane, c0 >> 3, &ptop);
                    wave_lds_sync();  // every lane has read the first pair's windows
                    mc_luma_wave(L.mcw, ref_y, g.pitch, g.coded_w, g.coded_h, 2, x0 * 4 + qx[2], y0 * 4 + qy[2],
                                 x0 * 4 + qx[3], y0 * 4 + qy[3], lane, c0 >> 3, &pbot);
                    pw = r < 8 ? ptop : pbot;
                    quad_mc = true;
                }
            }
        }
        if (quad_mc) {
            // pw is the prediction
        } else if ((vax | vay | vbx | vby) & 3) {
            // a fractional vector: interpolated from the block's window(s) staged in LDS
            const int lpi = part == kPart16x8 ? (r >> 3) : (part == kPart8x16 ? (c0 >> 3) : 0);
            mc_luma_wave(L.mcw, ref_y, g.pitch, g.coded_w, g.coded_h, part == kPart16x16 ? 1 : 2, x0 * 4 + vax,
                         y0 * 4 + vay, x0 * 4 + vbx, y0 * 4 + vby, lane, lpi, &pw);
        } else {
            // full-sample vectors (static desktop, scrolled text): 4 bytes of the reference row (edge
            // clamped), inside the picture from two aligned dwords instead of 4 byte gathers
            const int px = x0 + c0 + (mvx >> 2), py = min(max(y0 + r + (mvy >> 2), 0), g.coded_h - 1);
            if (px >= 0 && px + 4 <= g.coded_w && ((px & 3) == 0 || (px & ~3) + 8 <= g.pitch) && ref_dwords) {
                const uint32_t* qa = reinterpret_cast<const uint32_t*>(ref_y + (size_t)py * g.pitch + (px & ~3));
                const uint32_t sh = (uint32_t)(px & 3);
                pw = sh ? __builtin_amdgcn_alignbyte(qa[1], qa[0], sh) : qa[0];
            } else {
                for (int k = 0; k < 4; ++k)
                    pw |= (uint32_t)ref_px(ref_y, g.pitch, g.coded_w, g.coded_h, px + k, py) << (8 * k);
            }
        }
        lsad = (int)__builtin_amdgcn_sad_u8(sw, pw, 0u);
        const int cr_ = lane >> 3, cc = lane & 7;
        const int xc = x0 / 2 + cc, yc = y0 / 2 + cr_;
        const Mv cv = px_mv<kQuad>(mi, 2 * cc, 2 * cr_);
        for (int comp = 0; comp < 2; ++comp) {
            cpv[comp] = chroma_pred8(ref_uv, g.pitch, cw, ch, comp, xc * 8 + cv.x, yc * 8 + cv.y);
            crs[comp] = (int)src_uv[yc * g.pitch + 2 * xc + comp] - cpv[comp];
        }
    }
    const int aq = fs.aq;
    const bool want_cost = fs.intra_in_p != 0;  // MbInfo::cost (the SATD) is read by k_intra_analyze alone
    const uint32_t lsad_mb = (uint32_t)wave_sum(lsad);
    const int tcls = temporal_class((uint32_t)wave_sum(tsad), __ballot((mvx | mvy) != 0) == 0ull);
    const int qp = mb_qp_for(fs.qp, lsad_mb, tcls, aq);  // wave-uniform
    const int qpc = chroma_qp(qp, fs.chroma_qp_offset);
    int16_t* mc = coef + (size_t)mbi * kCoefStride;

    // ---- residuals known to quantise to zero (h264_mb.h zero_sum_4x4 / zero_sum_chroma_dc): the
    // macroblock's luma, or its chroma, then takes a shortcut that runs no transform -- levels 0,
    // reconstruction = prediction, distortion = sum residual^2 -- which is what the transforms give.
    // Both tests are wave-uniform.  Luma: a 4x4 block is lanes q, q + 4, q + 8, q + 12 of a row of 16.
    int bsum = lsad;
    bsum += __builtin_amdgcn_mov_dpp(bsum, 0x124, 0xF, 0xF, false);  // row_ror:4
    bsum += __builtin_amdgcn_mov_dpp(bsum, 0x128, 0xF, 0xF, false);  // row_ror:8
    const bool luma_zero = __ballot(bsum > zero_sum_4x4(qp)) == 0ull;
    // Chroma, U in the low and V in the high half-word (a plane sums to <= 64 * 255): block =
    // lanes that differ in bits 0, 1 (column) and 3, 4 (row); plane = also bits 2 and 5.
    int csum = abs(crs[0]) | (abs(crs[1]) << 16);
    csum += __builtin_amdgcn_mov_dpp(csum, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
    csum += __builtin_amdgcn_mov_dpp(csum, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
    csum += __builtin_amdgcn_mov_dpp(csum, 0x128, 0xF, 0xF, false);  // row_ror:8 = lane ^ 8
    {
        const auto r16 = __builtin_amdgcn_permlane16_swap((uint32_t)csum, (uint32_t)csum, false, false);
        csum = (int)(r16[0] + r16[1]);  // lane ^ 16
    }
    int psum = csum + __builtin_amdgcn_mov_dpp(csum, 0x124, 0xF, 0xF, false);  // row_ror:4: bit 2 flipped
    {
        const auto r32 = __builtin_amdgcn_permlane32_swap((uint32_t)psum, (uint32_t)psum, false, false);
        psum = (int)(r32[0] + r32[1]);  // lane ^ 32
    }
    const int zac = zero_sum_4x4(qpc), zdc = zero_sum_chroma_dc(qpc);
    const bool chroma_bound = __ballot((csum & 0xffff) > zac || (csum >> 16) > zac || (psum & 0xffff) > zdc ||
                                       (psum >> 16) > zdc) == 0ull;
    // the transforms' "row" layout goes through LDS; the shortcuts work on the load layout
    const bool luma_rows = !luma_zero || want_cost;
    if (luma_rows) {
        const int r = lane >> 2, c0 = (lane & 3) * 4;
        *reinterpret_cast<uint32_t*>(&L.pred[r * 16 + c0]) = pw;
        for (int k = 0; k < 4; ++k) L.res[r * 16 + c0 + k] = (int16_t)(byte_of(sw, k) - byte_of(pw, k));
    }
    if (!chroma_bound) {
        for (int comp = 0; comp < 2; ++comp) {
            L.pred[256 + comp * 64 + lane] = (uint8_t)cpv[comp];  // lane = 8 * row + column
            L.res[256 + comp * 64 + lane] = (int16_t)crs[comp];
        }
    }
    wave_lds_sync();

    // ---- luma: lane = 4 * blkIdx + row
    const int lb = lane >> 2, rr = lane & 3, lbx = kBlkX[lb], lby = kBlkY[lb];
    int x[4] = {0, 0, 0, 0};
    const int ro = (lby * 4 + rr) * 16 + lbx * 4;  // row offset in the MB's pred / res
    uint32_t satd_mb = 0;
    if (luma_rows) {
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = L.res[ro + c];
        if (want_cost) {
            const int hs = quad_sum(had_row_abs(x, rr));
            satd_mb = (uint32_t)wave_sum(rr == 0 ? (hs + 1) >> 1 : 0);
        }
    }
    bool drop = false;
    int nz_l = 0, sse_y = 0;
    if (luma_zero) {
        // No level of any block: cbp gets no luma bit, so no reader (k_cavlc's code_role) looks at
        // this macroblock's luma coefficients and none are stored.  drop_luma_for is false with a
        // bit estimate of 0.
        {
            const int r = lane >> 2, c0 = (lane & 3) * 4;
            const bool vis = x0 + c0 < g.width && (y0 + r) < g.height;
            for (int k = 0; k < 4; ++k) {
                const int e = byte_of(sw, k) - byte_of(pw, k);
                sse_y += vis ? e * e : 0;
            }
            *reinterpret_cast<uint32_t*>(fs.rec_y + (y0 + r) * g.pitch + x0 + c0) = pw;
            if (lane < 4) reinterpret_cast<uint32_t*>(mbs[mbi].nz_luma)[lane] = 0u;
        }
    } else {
        int y[4], z[4], rres[4];
        fdct_row(x, rr, y);
        const int nzb = quad_sum(quant_row(y, rr, qp, false, 0, z));
        {
            int d[4];
            dequant_row(z, rr, qp, d);
            idct_row(d, rr, rres);
        }
        if (drop_luma_possible(aq, lsad_mb, tcls)) {  // wave-uniform
            int d_pred = 0, d_coded = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int pv = L.pred[ro + c];
                const int e = pv + x[c] - clip255(pv + rres[c]);
                d_pred += x[c] * x[c];
                d_coded += e * e;
            }
            const uint32_t bits = rr == 0 ? block_bits_est(nzb) : 0u;
            drop = drop_luma_for(aq, lsad_mb, tcls, qp, wave_sum(d_pred), wave_sum(d_coded),
                                          (uint32_t)wave_sum((int)bits));
        }
        nz_l = drop ? 0 : nzb;
        {
            uint32_t packed = 0;
            const bool vis = x0 + lbx * 4 < g.width && (y0 + lby * 4 + rr) < g.height;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (drop) z[c] = rres[c] = 0;
                mc[kCoefLuma + lb * 16 + kZigzagInv4x4[rr * 4 + c]] = (int16_t)z[c];
                const int pv = L.pred[ro + c];
                const int v = clip255(pv + rres[c]);
                const int e = pv + x[c] - v;
                sse_y += vis ? e * e : 0;
                packed |= (uint32_t)v << (8 * c);
            }
            *reinterpret_cast<uint32_t*>(fs.rec_y + (y0 + lby * 4 + rr) * g.pitch + x0 + lbx * 4) = packed;
            if (rr == 0) mbs[mbi].nz_luma[lby * 4 + lbx] = (uint8_t)nz_l;
        }
    }
    const bool drop_c = drop_chroma_for(aq, tcls, drop);

    // ---- chroma: lanes 0..31, lane = 4 * (comp * 4 + blk) + row
    const int cbk = lane >> 2, ccomp = (cbk >> 2) & 1, cblk = cbk & 3, cbx = cblk & 1, cby = cblk >> 1;
    const int co = 256 + ccomp * 64 + (cby * 4 + rr) * 8 + cbx * 4;
    const bool clane = lane < 32;
    int nzc = 0, dc_any = 0;
    int sse_u = 0, sse_v = 0;  // this lane's share of the planes' distortion
    if (chroma_bound || drop_c) {
        // Every AC and DC level is 0 (a dropped macroblock codes no chroma residual either): cbp
        // gets chroma 0, so no reader looks at the chroma coefficients and none are stored.
        {
            const int xc = x0 / 2 + (lane & 7), yc = y0 / 2 + (lane >> 3);
            const bool vis = 2 * xc < g.width && 2 * yc < g.height;
            sse_u = vis ? crs[0] * crs[0] : 0;
            sse_v = vis ? crs[1] * crs[1] : 0;
            uint8_t* o = fs.rec_uv + yc * g.pitch + 2 * xc;
            if (((reinterpret_cast<uintptr_t>(fs.rec_uv) | (uintptr_t)g.pitch) & 1) == 0) {
                *reinterpret_cast<uint16_t*>(o) = (uint16_t)(cpv[0] | (cpv[1] << 8));
            } else {
                o[0] = (uint8_t)cpv[0];
                o[1] = (uint8_t)cpv[1];
            }
            if (lane < 2) reinterpret_cast<uint32_t*>(mbs[mbi].nz_cb)[lane] = 0u;  // nz_cb, nz_cr
        }
    } else {
        int cz[4];
        if (clane) {
            int cx[4], cy[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) cx[c] = L.res[co + c];
            fdct_row(cx, rr, cy);
            if (rr == 0) L.cdc[ccomp * 4 + cblk] = cy[0];
            nzc = quant_row(cy, rr, qpc, false, 1, cz);
        }
        nzc = quad_sum(nzc);
        if (clane) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int i = rr * 4 + c;
                if (i > 0) mc[kCoefChromaAc + (ccomp * 4 + cblk) * 16 + kZigzagInv4x4[i]] = (int16_t)cz[c];
            }
            if (rr == 0) (ccomp ? mbs[mbi].nz_cr : mbs[mbi].nz_cb)[cblk] = (uint8_t)nzc;
        }
        wave_lds_sync();
        if ((lane == 0 || lane == 16)) {
            const int comp = lane >> 4;
            int in[4], zd[4], dq[4];
            for (int i = 0; i < 4; ++i) in[i] = L.cdc[comp * 4 + i];
            const int n = quant_dc_chroma(in, zd, qpc, false);
            for (int i = 0; i < 4; ++i) mc[kCoefChromaDc + comp * 4 + i] = (int16_t)zd[i];
            dequant_dc_chroma(zd, dq, qpc);
            for (int i = 0; i < 4; ++i) L.cdc[comp * 4 + i] = dq[i];
            L.cdc_nz[comp] = n;
        }
        wave_lds_sync();
        if (clane) {
            int d[4], cr[4];
            dequant_row(cz, rr, qpc, d);
            if (rr == 0) d[0] = L.cdc[ccomp * 4 + cblk];
            idct_row(d, rr, cr);
            {
                const int xc = x0 / 2 + cbx * 4, yc = y0 / 2 + cby * 4 + rr;
                int sse_c = 0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int v = clip255(L.pred[co + c] + cr[c]);
                    const int e = L.pred[co + c] + L.res[co + c] - v;
                    sse_c += (2 * (xc + c) < g.width && 2 * yc < g.height) ? e * e : 0;
                    fs.rec_uv[yc * g.pitch + 2 * (xc + c) + ccomp] = (uint8_t)v;
                }
                (ccomp ? sse_v : sse_u) = sse_c;  // U on lanes 0..15, V on 16..31
            }
        }
        dc_any = L.cdc_nz[0] | L.cdc_nz[1];
    }
    {
        const int sy = wave_sum(sse_y);
        const int su = wave_sum(sse_u);
        const int sv = wave_sum(sse_v);
        if (lane < 3) mb_sse[lane * nmb + mbi] = (uint32_t)(lane == 0 ? sy : (lane == 1 ? su : sv));
    }
    const unsigned long long luma_mask = __ballot(rr == 0 && nz_l > 0);    // bit 4b: block b
    const unsigned long long chroma_mask = __ballot(clane && rr == 0 && nzc > 0);
    if (lane == 0) {
        int cbp = 0;
        for (int b8 = 0; b8 < 4; ++b8)
            if ((luma_mask >> (16 * b8)) & 0x1111ull) cbp |= 1 << b8;
        const int cc = (chroma_mask != 0) ? 2 : (dc_any ? 1 : 0);
        cbp |= cc << 4;
        MbInfo& m = mbs[mbi];
        m.type = kMbP16x16;
        m.cbp = (uint8_t)cbp;
        m.qp = (uint8_t)qp;
        m.i16_mode = 0;
        m.chroma_mode = 0;
        m.cost = want_cost ? inter_cost_mb<kQuad>(satd_mb, fs.qp, mi) : 0u;
    }
}

// The coder as a kernel of its own (a picture whose search ran beside the reference's in-loop
// filter): four macroblocks per workgroup, a wave each, independent of one another.
__global__ __launch_bounds__(256) void k_inter_encode(Geometry g, const FrameState* __restrict__ fs,
                                                       const uint8_t* __restrict__ src_y,
                                                       const uint8_t* __restrict__ src_uv, MbInfo* __restrict__ mbs,
                                                       int16_t* __restrict__ coef, uint32_t* __restrict__ mb_sse,
                                                       int* __restrict__ wave_prog) {
    __shared__ InterLds lds[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int mbi = blockIdx.x * 4 + wave;
    if (blockIdx.x == 0 && threadIdx.x == 0) wave_prog[1] = 0;  // k_intra_analyze's candidate list (next kernel)
    if (mbi >= g.mb_w * g.mb_h) return;  // the whole wave
    const MbInfo mi = mbs[mbi];
    inter_code_mb(g, code_state(*fs), src_y, src_uv, mbs, coef, mb_sse, mbi, lane, mi, lds[wave]);
}
// The same for a picture that may hold P_8x8 macroblocks (EncoderConfig::partitions 2)
__global__ __launch_bounds__(256) void k_inter_encode_q8(Geometry g, const FrameState* __restrict__ fs,
                                                          const uint8_t* __restrict__ src_y,
                                                          const uint8_t* __restrict__ src_uv, MbInfo* __restrict__ mbs,
                                                          int16_t* __restrict__ coef, uint32_t* __restrict__ mb_sse,
                                                          int* __restrict__ wave_prog) {
    __shared__ InterLds lds[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int mbi = blockIdx.x * 4 + wave;
    if (blockIdx.x == 0 && threadIdx.x == 0) wave_prog[1] = 0;  // k_intra_analyze's candidate list (next kernel)
    if (mbi >= g.mb_w * g.mb_h) return;  // the whole wave
    const MbInfo mi = mbs[mbi];
    inter_code_mb<true>(g, code_state(*fs), src_y, src_uv, mbs, coef, mb_sse, mbi, lane, mi, lds[wave]);
}

// One kernel per P picture whose search reads the picture the coder predicts from: a workgroup per
// macroblock searches as k_me_full does, then its wave 0 codes the macroblock with the vectors just
// decided while the other waves leave.  The coder's LDS lies over the search window, which nobody
// reads any more by then.  The first kernel of the picture: publishes the frame state (StateArg).
// (6 waves per SIMD asked for: left alone the allocation ends one register over that step)
__global__ __launch_bounds__(kMeThreads) __attribute__((amdgpu_waves_per_eu(6))) void k_p_fused(Geometry g, StateArg sa, const uint8_t* __restrict__ src_y,
                                                        const uint8_t* __restrict__ src_uv, MbInfo* __restrict__ mbs,
                                                        int16_t* __restrict__ coef, uint32_t* __restrict__ mb_sse,
                                                        int* __restrict__ wave_prog) {
    __shared__ uint32_t win_lds[kWinWords];
    static_assert(sizeof(InterLds) <= sizeof(uint32_t) * kWinWords, "the coder's LDS aliases the search window");
    publish_state(sa);
    if (blockIdx.x == 0 && threadIdx.x == 0) wave_prog[1] = 0;  // k_intra_analyze's candidate list (next kernel)
    const MeState st = sa.publish ? me_state(sa.v) : me_state(*sa.dst);
    const CodeState cs = sa.publish ? code_state(sa.v) : code_state(*sa.dst);
    const MbInfo mi = me_full_body<false>(g, st, src_y, mbs, win_lds);  // the same on every thread
    __syncthreads();  // every wave is done with the window
    if (threadIdx.x >= 64) return;
    inter_code_mb(g, cs, src_y, src_uv, mbs, coef, mb_sse, blockIdx.x, threadIdx.x, mi,
                  *reinterpret_cast<InterLds*>(win_lds));
}
// The same with the scroll hint (after k_scroll_probe, which stamped the start); a kernel of its own,
// so that k_p_fused keeps its registers
__global__ __launch_bounds__(kMeThreads) __attribute__((amdgpu_waves_per_eu(6))) void k_p_fused_scroll(
    Geometry g, StateArg sa, const uint8_t* __restrict__ src_y, const uint8_t* __restrict__ src_uv,
    MbInfo* __restrict__ mbs, int16_t* __restrict__ coef, uint32_t* __restrict__ mb_sse, int* __restrict__ wave_prog,
    const int32_t* __restrict__ hint) {
    __shared__ uint32_t win_lds[kWinWords];
    static_assert(sizeof(InterLds) <= sizeof(uint32_t) * kWinWords, "the coder's LDS aliases the search window");
    publish_state(sa);
    if (blockIdx.x == 0 && threadIdx.x == 0) wave_prog[1] = 0;  // k_intra_analyze's candidate list (next kernel)
    const MeState st = sa.publish ? me_state(sa.v) : me_state(*sa.dst);
    const CodeState cs = sa.publish ? code_state(sa.v) : code_state(*sa.dst);
    const MbInfo mi = me_full_body<true>(g, st, src_y, mbs, win_lds, hint);  // the same on every thread
    __syncthreads();  // every wave is done with the window
    if (threadIdx.x >= 64) return;
    inter_code_mb(g, cs, src_y, src_uv, mbs, coef, mb_sse, blockIdx.x, threadIdx.x, mi,
                  *reinterpret_cast<InterLds*>(win_lds));
}
// k_p_fused and k_p_fused_scroll with the 8x8 quadrants searched and P_8x8 coded
// (EncoderConfig::partitions 2): kernels of their own, as the scroll ones are.  5 waves per SIMD asked
// for: the eight extra running bests need ~100 registers; at 6 waves the spills cost more than the
// occupancy returns and left alone the allocation ends at 4 (1080p desktop: 78.5 / 69.6 / 74.1 us for
// 6 / 5 / no limit, profiles/p8x8/NOTES.md)
template <bool kScroll>
__device__ __forceinline__ void p_fused_q8_body(const Geometry& g, const StateArg& sa, const uint8_t* __restrict__ src_y,
                                                const uint8_t* __restrict__ src_uv, MbInfo* __restrict__ mbs,
                                                int16_t* __restrict__ coef, uint32_t* __restrict__ mb_sse,
                                                int* __restrict__ wave_prog, const int32_t* __restrict__ hint,
                                                uint32_t* win_lds) {
    publish_state(sa);
    if (blockIdx.x == 0 && threadIdx.x == 0) wave_prog[1] = 0;  // k_intra_analyze's candidate list (next kernel)
    const MeState st = sa.publish ? me_state(sa.v) : me_state(*sa.dst);
    const CodeState cs = sa.publish ? code_state(sa.v) : code_state(*sa.dst);
    const MbInfo mi = me_full_body<kScroll, true>(g, st, src_y, mbs, win_lds, hint);  // the same on every thread
    __syncthreads();  // every wave is done with the window
    if (threadIdx.x >= 64) return;
    inter_code_mb<true>(g, cs, src_y, src_uv, mbs, coef, mb_sse, blockIdx.x, threadIdx.x, mi,
                        *reinterpret_cast<InterLds*>(win_lds));
}
__global__ __launch_bounds__(kMeThreads) __attribute__((amdgpu_waves_per_eu(5))) void k_p_fused_q8(
    Geometry g, StateArg sa, const uint8_t* __restrict__ src_y, const uint8_t* __restrict__ src_uv,
    MbInfo* __restrict__ mbs, int16_t* __restrict__ coef, uint32_t* __restrict__ mb_sse, int* __restrict__ wave_prog) {
    __shared__ uint32_t win_lds[kWinWords];
    p_fused_q8_body<false>(g, sa, src_y, src_uv, mbs, coef, mb_sse, wave_prog, nullptr, win_lds);
}
__global__ __launch_bounds__(kMeThreads) __attribute__((amdgpu_waves_per_eu(5))) void k_p_fused_scroll_q8(
    Geometry g, StateArg sa, const uint8_t* __restrict__ src_y, const uint8_t* __restrict__ src_uv,
    MbInfo* __restrict__ mbs, int16_t* __restrict__ coef, uint32_t* __restrict__ mb_sse, int* __restrict__ wave_prog,
    const int32_t* __restrict__ hint) {
    __shared__ uint32_t win_lds[kWinWords];
    p_fused_q8_body<true>(g, sa, src_y, src_uv, mbs, coef, mb_sse, wave_prog, hint, win_lds);
}

// ------------------------------------------------------------------ intra analysis
// raster block index -> blkIdx
__constant__ uint8_t kRasterToBlk[16] = {0, 1, 4, 5, 2, 3, 6, 7, 8, 9, 12, 13, 10, 11, 14, 15};

// One wave per macroblock, fully parallel: SATD of the 9 Intra4x4 modes of the 16 blocks
// (144 block/mode pairs over 64 lanes), of the 4 Intra16x16 modes (one 4x4 block per lane)
// and of the 4 chroma modes, all predicted from SOURCE neighbours (open loop), then the
// shared decide_intra() on lane 0.  IDR: every MB takes its decision; P: only MBs whose
// intra cost beats the inter cost k_inter_encode left in MbInfo::cost.  Block 0 also resets
// k_intra_wave's progress counters and row ticket.
constexpr int kLT = 24;  // luma LDS tile pitch: x -1 .. 19 at columns 0 .. 20 (rows y -1 .. 15)
constexpr int kCT = 10;  // chroma LDS tile pitch (per plane): x -1 .. 7 at columns 0 .. 8
constexpr int kCTI = 20; // interleaved chroma LDS tile pitch: (x -1 .. 8) x 2 planes

__global__ __launch_bounds__(256) void k_intra_analyze(Geometry g, StateArg sa, const uint8_t* __restrict__ src_y,
                                                       const uint8_t* __restrict__ src_uv, MbInfo* __restrict__ mbs,
                                                       int* __restrict__ wave_prog, int32_t* __restrict__ gain,
                                                       int* __restrict__ cand) {
    __shared__ IntraCosts costs[4];
    __shared__ uint8_t ltile[4][17][kLT];   // source luma: MB + one-sample border + top-right
    __shared__ uint8_t ctile[4][9][kCTI];   // source chroma (interleaved): MB + one-sample border
    publish_state(sa);
    const FrameState* fs = &state_of(sa);
    if (blockIdx.x == 0) {
        if (!fs->idr)  // k_intra_p's per-row distortion deltas (atomically accumulated)
            for (int i = threadIdx.x; i < 4 * g.mb_h; i += 256)
                fs->sse_part[(i / g.mb_h) * kSsePartStride + i % g.mb_h] = 0;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int mbi = blockIdx.x * 4 + wave;
    if (mbi >= g.mb_w * g.mb_h) return;  // whole wave; no workgroup barriers below
    if (!fs->idr && !intra_candidate(mbs[mbi].cost)) {  // well-predicted: stays inter
        if (lane == 0) gain[mbi] = 0;
        return;
    }
    const int mbx = mbi % g.mb_w, mby = mbi / g.mb_w;
    const int x0 = mbx * 16, y0 = mby * 16;
    const Avail av = mb_avail(g, mbx, mby, fs->slice_rows);
    // stage the source footprint (samples outside the picture are never read: availability)
    for (int i = lane; i < 17 * 21; i += 64) {
        const int r = i / 21, cx = i - r * 21, x = x0 - 1 + cx, y = y0 - 1 + r;
        ltile[wave][r][cx] = (x >= 0 && y >= 0 && x < g.coded_w) ? src_y[y * g.pitch + x] : 0;
    }
    for (int i = lane; i < 9 * 18; i += 64) {
        const int r = i / 18, bx = i - r * 18, x = x0 - 2 + bx, y = y0 / 2 - 1 + r;
        ctile[wave][r][bx] = (x >= 0 && y >= 0) ? src_uv[y * g.pitch + x] : 0;
    }
    wave_lds_sync();
    const uint8_t* sy = &ltile[wave][1][1];
    const uint8_t* suv = &ctile[wave][1][2];
    IntraCosts& c = costs[wave];
    // lane = (4x4 block, row): every mode is evaluated by the whole wave at once (a per-lane
    // mode would diverge the prediction switch 9 ways), SATD as row Hadamards in registers plus
    // a column butterfly over the block's 4 lanes; the same integers as satd4x4().
    const int rb = lane >> 2, r = lane & 3, bx = rb & 3, by = rb >> 2;
    auto satd_quad = [&](int d0, int d1, int d2, int d3) -> uint32_t {
        int t[4] = {d0 + d1 + d2 + d3, d0 + d1 - d2 - d3, d0 - d1 - d2 + d3, d0 - d1 + d2 - d3};
        uint32_t sum = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // column butterflies over the quad: DPP quad_perm xor 1 / xor 2
            int v = t[j];
            int o = __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, false);
            v = (r & 1) ? o - v : v + o;
            o = __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, false);
            v = (r & 2) ? o - v : v + o;
            sum += (uint32_t)(v < 0 ? -v : v);
        }
        sum += (uint32_t)__builtin_amdgcn_mov_dpp((int)sum, 0xB1, 0xF, 0xF, false);
        sum += (uint32_t)__builtin_amdgcn_mov_dpp((int)sum, 0x4E, 0xF, 0xF, false);
        return (sum + 1) >> 1;  // satd of the block, in all 4 lanes
    };
    {
        const Nb4 n = nb4_from_plane(sy, kLT, 0, 0, bx, by, av.left, av.top, av.topright, av.topleft);
        int sv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) sv[j] = sy[(4 * by + r) * kLT + 4 * bx + j];
        for (int m = 0; m < 9; ++m) {
            const bool ok = i4_mode_ok(m, n);
            int d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = ok ? sv[j] - pred4x4_px(m, n, j, r) : 0;
            const uint32_t t = satd_quad(d[0], d[1], d[2], d[3]);
            if (r == 0) c.c4[kRasterToBlk[rb]][m] = ok ? t : kCostInf;
        }
    }
    {  // Intra16x16: 4 modes, all 16 blocks at once, summed over the wave
        const NbMb n = nbmb_from_plane(sy, kLT, 0, 0, 16, 1, 0, av.left, av.top, av.topleft);
        for (int m = 0; m < 4; ++m) {
            const bool ok = i16_mode_ok(m, n);  // wave-uniform
            uint32_t t = 0;
            if (ok) {
                const PredMb p = prep_i16(m, n);
                int d[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    d[j] = (int)sy[(4 * by + r) * kLT + 4 * bx + j] - pred16_px(p, n, 4 * bx + j, 4 * by + r);
                t = satd_quad(d[0], d[1], d[2], d[3]);
                t = r == 0 ? t : 0u;
                t += (uint32_t)__builtin_amdgcn_mov_dpp((int)t, 0x124, 0xF, 0xF, false);  // lanes l ^ 4, 8, 12
                t += (uint32_t)__builtin_amdgcn_mov_dpp((int)t, 0x128, 0xF, 0xF, false);
                t = rows_sum(t);
            }
            if (lane == 0) c.c16[m] = ok ? t : kCostInf;
        }
    }
    {  // chroma: 4 modes; lanes 0..31 = (component, 4x4 block, row), lanes 32..63 idle
        const int comp = (lane >> 4) & 1, cb = (lane >> 2) & 3, cbx = cb & 1, cby = cb >> 1;
        const NbMb n = nbmb_from_plane(suv, kCTI, 0, 0, 8, 2, comp, av.left, av.top, av.topleft);
        for (int m = 0; m < 4; ++m) {
            const bool ok = chroma_mode_ok(m, n);  // wave-uniform (same availability for both planes)
            uint32_t t = 0;
            if (ok) {
                const PredMb p = prep_chroma(m, n);
                int d[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    d[j] = lane < 32 ? (int)suv[(4 * cby + r) * kCTI + 2 * (4 * cbx + j) + comp] -
                                           predc_px(p, n, 4 * cbx + j, 4 * cby + r)
                                     : 0;
                t = satd_quad(d[0], d[1], d[2], d[3]);
                t = (r == 0 && lane < 32) ? t : 0u;
                t += (uint32_t)__builtin_amdgcn_mov_dpp((int)t, 0x124, 0xF, 0xF, false);  // lanes l ^ 4, 8, 12
                t += (uint32_t)__builtin_amdgcn_mov_dpp((int)t, 0x128, 0xF, 0xF, false);
                t = rows_sum(t);
            }
            if (lane == 0) c.cc[m] = ok ? t : kCostInf;
        }
    }
    wave_lds_sync();
    if (lane == 0) {
        const IntraDecision d = decide_intra(c, fs->qp, fs->intra4x4 != 0);
        MbInfo& m = mbs[mbi];
        const int32_t gn = fs->idr ? 1 : intra_gain(d.cost_luma, m.cost, fs->qp);
        if (!fs->idr) {
            gain[mbi] = gn;
            if (gn > 0) cand[atomicAdd(&wave_prog[1], 1)] = mbi;  // k_intra_p's work list
        }
        if (gn > 0) {  // IDR: the decision; P: a pending decision, applied by k_intra_p if selected
            const int qp = fs->qp;
            if (fs->idr)
                m.type = (uint8_t)d.type;
            else
                m.itype = (uint8_t)d.type;
            m.i16_mode = (uint8_t)d.i16_mode;
            m.chroma_mode = (uint8_t)d.chroma_mode;
            uint8_t md[8];
            for (int rb = 0; rb < 16; rb += 2) md[rb >> 1] = (uint8_t)(d.i4[rb] | (d.i4[rb + 1] << 4));
            for (int k = 0; k < 8; ++k) m.i4[k] = md[k];
            if (fs->idr) {
                m.qp = (uint8_t)qp;
                m.mvx = 0;
                m.mvy = 0;
            }
        }
    }
}

// ------------------------------------------------------------------ intra reconstruction
// Closed-loop coding of the intra macroblocks in a diagonal wavefront.  One workgroup per MB
// row (row order taken from a ticket counter, so a row only ever waits on rows that are
// already running); wave 0 codes luma, wave 1 chroma -- the two planes' intra predictions
// are independent, so they run as two wavefronts.  A macroblock waits until the row above
// (same slice) has finished the macroblock above-right (per-plane progress counters,
// agent-scope release / acquire).  Neighbour samples are staged in LDS tiles with a one-
// sample border; the prediction helpers read them through the same plane-accessors as the
// CPU encoder, so decisions and reconstructions are bit-identical.
//  * Intra4x4: the 16 blocks in 10 dependency steps (block (bx,by) at step bx + 2*by, up to
//    two blocks per step), one pixel per lane; the 4x4 transforms run as row / column
//    butterflies over lane shuffles within each 16-lane block group.
//  * Intra16x16 and chroma: one 4x4 block per lane, DC transforms on one lane.
// In P pictures the waves skip inter macroblocks (final since k_inter_encode) and replace the
// inter distortion of the switched macroblocks by a per-row delta partial.


// Per-MB fields the reconstruction needs, read once (prefetched a macroblock ahead).
struct MbFields {
    int type, qp, i16_mode, chroma_mode;
    uint32_t i4lo, i4hi;  // Intra4x4 modes, nibbles in raster block order
    __device__ int i4(int rb) const { return (int)(((rb < 8 ? i4lo : i4hi) >> (4 * (rb & 7))) & 15u); }
};
__device__ __forceinline__ MbFields load_fields(const MbInfo* m) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(m);  // MbInfo: 48 B, dword aligned
    const uint32_t d1 = w[1], d8 = w[8], d9 = w[9], d10 = w[10];
    MbFields f;
    f.type = (int)(d1 & 0xff);
    f.i16_mode = (int)((d1 >> 16) & 0xff);
    f.chroma_mode = (int)(d1 >> 24);
    f.qp = (int)((d8 >> 8) & 0xff);
    f.i4lo = d9;
    f.i4hi = d10;
    return f;
}
static_assert(offsetof(MbInfo, type) == 4 && offsetof(MbInfo, i16_mode) == 6 && offsetof(MbInfo, chroma_mode) == 7 &&
                  offsetof(MbInfo, qp) == 33 && offsetof(MbInfo, i4) == 36,
              "load_fields() layout");


// Quantiser constants of one QP, read with wave-uniform indices (scalar loads) and picked per
// coefficient position with selects: a lane-indexed table read is a vector memory round trip,
// and in the wavefront every one of them sits on the critical path (profiles/r02_idr).
struct QpTab {
    int mf0, mf1, mf2;  // kQuantMF[qp % 6][class]
    int dv0, dv1, dv2;  // kDequantV[qp % 6][class]
    int qbits, qs;
    uint32_t f_intra;
    __device__ int mf(int cls) const { return cls == 0 ? mf0 : (cls == 1 ? mf1 : mf2); }
    __device__ int dv(int cls) const { return cls == 0 ? dv0 : (cls == 1 ? dv1 : dv2); }
};
__device__ __forceinline__ QpTab qp_tab(int qp) {
    QpTab t;
    const int qm = qp % 6;
    t.mf0 = kQuantMF[qm][0];
    t.mf1 = kQuantMF[qm][1];
    t.mf2 = kQuantMF[qm][2];
    t.dv0 = kDequantV[qm][0];
    t.dv1 = kDequantV[qm][1];
    t.dv2 = kDequantV[qm][2];
    t.qbits = 15 + qp / 6;
    t.qs = qp / 6;
    t.f_intra = (1u << t.qbits) / 3;
    return t;
}
// kPosClass of raster position (r, c): 0 both even, 1 both odd, 2 mixed
__device__ __forceinline__ int pos_class(int r, int c) { return ((r | c) & 1) == 0 ? 0 : (((r & c) & 1) ? 1 : 2); }
// kZigzagInv4x4 as nibbles of one 64-bit immediate
constexpr uint64_t zz_inv_packed() {
    uint64_t v = 0;
    for (int i = 0; i < 16; ++i) v |= (uint64_t)kZigzagInv4x4[i] << (4 * i);
    return v;
}
__device__ __forceinline__ int zz_inv(int i) { return (int)((zz_inv_packed() >> (4 * i)) & 15u); }
// blkIdx <-> raster 4x4 block position (6.4.3), arithmetic
__device__ __forceinline__ int blk_x(int b) { return (b & 1) | ((b >> 1) & 2); }
__device__ __forceinline__ int blk_y(int b) { return ((b >> 1) & 1) | ((b >> 2) & 2); }
// Intra4x4 schedule: raster block of quad group `grp` (0, 1) at dependency step t (block
// (bx, by) at step bx + 2 by), -1 if none
__device__ __forceinline__ int i4_step_block(int t, int grp) {
    const int by = (t >= 2 ? (t - 2) >> 1 : 0) + grp, bx = t - 2 * by;
    return (bx >= 0 && bx <= 3 && by <= 3) ? by * 4 + bx : -1;
}
__device__ __forceinline__ int raster_to_blk(int rb) {
    const int bx = rb & 3, by = rb >> 2;
    return ((by >> 1) << 3) | ((bx >> 1) << 2) | ((by & 1) << 1) | (bx & 1);
}
// quant4x4 / dequant4x4 of row r (intra rounding), 32-bit: |y| * MF + f < 2^31 for 8-bit video
__device__ __forceinline__ int quant_row_i(const int* y, int r, const QpTab& t, int start, int* z) {
    int nz = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int a = y[c] < 0 ? -y[c] : y[c];
        int q = (int)(((uint32_t)a * (uint32_t)t.mf(pos_class(r, c)) + t.f_intra) >> t.qbits);
        q = q > kMaxLevel ? kMaxLevel : q;
        q = (r * 4 + c) < start ? 0 : q;
        z[c] = y[c] < 0 ? -q : q;
        nz += (q != 0);
    }
    return nz;
}
__device__ __forceinline__ void dequant_row_t(const int* z, int r, const QpTab& t, int* d) {
#pragma unroll
    for (int c = 0; c < 4; ++c) d[c] = z[c] * t.dv(pos_class(r, c)) * (1 << t.qs);
}
// Hadamard of row r of a 4x4 block whose rows sit in the quad (hadamard4x4, rows then columns)
__device__ __forceinline__ void had_row(const int* x, int r, int* y) {
    const int t[4] = {x[0] + x[1] + x[2] + x[3], x[0] + x[1] - x[2] - x[3], x[0] - x[1] - x[2] + x[3],
                      x[0] - x[1] + x[2] - x[3]};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int a = qbc<0>(t[c]), b = qbc<1>(t[c]), cc = qbc<2>(t[c]), d = qbc<3>(t[c]);
        y[c] = r == 0 ? a + b + cc + d : r == 1 ? a + b - cc - d : r == 2 ? a - b - cc + d : a - b + cc - d;
    }
}

// The 4 prediction samples of row r of an Intra4x4 block: one switch on the mode per row
// (the per-sample pred4x4_px switch, unrolled over the row, evaluated 4 mode switches with
// the quads' different modes as divergent branch chains); same formulas, constant-folded.
template <int M>
__device__ __forceinline__ void pred4x4_row_m(const Nb4& n, int r, int* pv) {
#pragma unroll
    for (int c = 0; c < 4; ++c) pv[c] = pred4x4_px(M, n, c, r);
}
__device__ __forceinline__ void pred4x4_row(int mode, const Nb4& n, int r, int* pv) {
    switch (mode) {
        case 0: pred4x4_row_m<0>(n, r, pv); break;
        case 1: pred4x4_row_m<1>(n, r, pv); break;
        case 2: pred4x4_row_m<2>(n, r, pv); break;
        case 3: pred4x4_row_m<3>(n, r, pv); break;
        case 4: pred4x4_row_m<4>(n, r, pv); break;
        case 5: pred4x4_row_m<5>(n, r, pv); break;
        case 6: pred4x4_row_m<6>(n, r, pv); break;
        case 7: pred4x4_row_m<7>(n, r, pv); break;
        default: pred4x4_row_m<8>(n, r, pv); break;
    }
}

// Intra16x16 / chroma prediction of 4 samples of one row, the mode switch hoisted out of the row
template <int M, bool C>
__device__ __forceinline__ void predmb_row_m(const PredMb& p, const NbMb& n, int x0, int y, int* pv) {
    PredMb q = p;
    q.mode = M;  // constant mode: the helpers' switches fold
#pragma unroll
    for (int c = 0; c < 4; ++c) pv[c] = C ? predc_px(q, n, x0 + c, y) : pred16_px(q, n, x0 + c, y);
}
template <bool C>
__device__ __forceinline__ void predmb_row(const PredMb& p, const NbMb& n, int x0, int y, int* pv) {
    switch (p.mode) {
        case 0: predmb_row_m<0, C>(p, n, x0, y, pv); break;
        case 1: predmb_row_m<1, C>(p, n, x0, y, pv); break;
        case 2: predmb_row_m<2, C>(p, n, x0, y, pv); break;
        default: predmb_row_m<3, C>(p, n, x0, y, pv); break;
    }
}

// One Intra4x4 block on a quad (row r on this lane): predict from the tile, transform,
// quantise, store the levels, reconstruct into the tile.  Returns the block's level count.
__device__ __forceinline__ int i4_code_block(const Geometry& g, int rb, int r, int mode, const QpTab& T,
                                             const uint32_t* ls, uint8_t (*lt)[kLT], int16_t* __restrict__ mc, int x0,
                                             int y0, const Avail& av, uint32_t& sse) {
    const uint8_t* tile = &lt[1][1];
    const int bx = rb & 3, by = rb >> 2, py = 4 * by + r;
    const Nb4 n = nb4_from_plane(tile, kLT, 0, 0, bx, by, av.left, av.top, av.topright, av.topleft);
    const uint32_t sw = ls[py * 4 + bx];
    int pv[4], x[4], y[4], z[4], d[4], rr[4];
    pred4x4_row(mode, n, r, pv);
#pragma unroll
    for (int c = 0; c < 4; ++c) x[c] = (int)((sw >> (8 * c)) & 0xff) - pv[c];
    fdct_row(x, r, y);
    const int nzb = quad_sum(quant_row_i(y, r, T, 0, z));
    const int b = raster_to_blk(rb);
#pragma unroll
    for (int c = 0; c < 4; ++c) mc[kCoefLuma + b * 16 + zz_inv(r * 4 + c)] = (int16_t)z[c];
    dequant_row_t(z, r, T, d);
    idct_row(d, r, rr);
    const bool vis = y0 + py < g.height;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int rec = clip255(pv[c] + rr[c]);
        lt[1 + py][1 + 4 * bx + c] = (uint8_t)rec;
        const int e = x[c] + pv[c] - rec;
        sse += (vis && x0 + 4 * bx + c < g.width) ? (uint32_t)(e * e) : 0u;
    }
    return nzb;
}

// Closed-loop coding of one intra macroblock's luma, in the 4x4 "row" layout of
// k_inter_encode (lane 4b + r = row r of block b): every transform pass is in-lane or a DPP
// quad broadcast, the quantiser tables are scalar.  ls: the MB's source luma (16 rows x 4
// dwords); lt: the LDS tile with the neighbours at row 0 / column 0, reconstructed in place.
//  * Intra4x4: the 16 blocks in 10 dependency steps (block (bx,by) at step bx + 2*by, up to
//    two blocks = two quads per step).
//  * Intra16x16: all 16 blocks at once; the DC Hadamard / quantiser on quad 0 (row layout of
//    the 4x4 DC matrix).
__device__ void intra_luma_mb(const Geometry& g, const MbFields& f, const uint32_t* ls, MbInfo& m,
                              int16_t* __restrict__ mc, int mbx, int mby, const Avail& av, uint8_t (*lt)[kLT],
                              int* ldc, int lane, uint32_t& sse) {
    const int x0 = mbx * 16, y0 = mby * 16;
    const QpTab T = qp_tab(f.qp);
    const uint8_t* tile = &lt[1][1];
    const int r = lane & 3;
    int cbp_l = 0;
    if (f.type == kMbI4x4) {
        const int grp = lane >> 2;
        for (int t = 0; t < 10; ++t) {
            const int rb = grp < 2 ? i4_step_block(t, grp) : -1;  // uniform per quad
            int nzb = 0;
            if (rb >= 0) {
                nzb = i4_code_block(g, rb, r, f.i4(rb), T, ls, lt, mc, x0, y0, av, sse);
                if (r == 0) m.nz_luma[rb] = (uint8_t)nzb;
            }
            const unsigned long long any = __ballot(rb >= 0 && r == 0 && nzb > 0);
            for (int gq = 0; gq < 2; ++gq)
                if ((any >> (4 * gq)) & 1ull) cbp_l |= 1 << (raster_to_blk(i4_step_block(t, gq)) >> 2);
            wave_lds_sync();
        }
    } else {  // Intra16x16
        const NbMb n = nbmb_from_plane(tile, kLT, 0, 0, 16, 1, 0, av.left, av.top, av.topleft);
        const PredMb p = prep_i16(f.i16_mode, n);
        const int b = lane >> 2, bx = blk_x(b), by = blk_y(b), py = 4 * by + r;
        const uint32_t sw = ls[py * 4 + bx];
        int pv[4], x[4], y[4], z[4];
        predmb_row<false>(p, n, 4 * bx, py, pv);
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = (int)((sw >> (8 * c)) & 0xff) - pv[c];
        fdct_row(x, r, y);
        if (r == 0) ldc[by * 4 + bx] = y[0];
        const int nz = quad_sum(quant_row_i(y, r, T, 1, z));
#pragma unroll
        for (int c = 0; c < 4; ++c) mc[kCoefLuma + b * 16 + zz_inv(r * 4 + c)] = (int16_t)z[c];
        wave_lds_sync();
        if (lane < 4) {  // DC matrix row `lane`: Hadamard, /2, quantise (quant_dc_luma), then dequant_dc_luma
            int dc[4], h[4], zd[4], fh[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) dc[c] = ldc[lane * 4 + c];
            had_row(dc, lane, h);
            const uint32_t qb = (uint32_t)(T.qbits + 1), fd = 2u * ((1u << (qb - 1)) / 3);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int v = h[c] >> 1;
                const int a = v < 0 ? -v : v;
                int q = (int)(((uint32_t)a * (uint32_t)T.mf0 + fd) >> qb);
                q = q > kMaxLevel ? kMaxLevel : q;
                zd[c] = v < 0 ? -q : q;
                mc[kCoefLumaDc + zz_inv(lane * 4 + c)] = (int16_t)zd[c];
            }
            had_row(zd, lane, fh);
            const int ls16 = 16 * T.dv0;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                ldc[lane * 4 + c] = f.qp >= 36 ? fh[c] * ls16 * (1 << (T.qs - 6))
                                               : (fh[c] * ls16 + (1 << (5 - T.qs))) >> (6 - T.qs);
        }
        wave_lds_sync();
        const bool luma_ac = __ballot(r == 0 && nz > 0) != 0;
        int d[4], rr[4];
        dequant_row_t(z, r, T, d);
        if (r == 0) d[0] = ldc[by * 4 + bx];
        idct_row(d, r, rr);
        const bool vis = y0 + py < g.height;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int rec = clip255(pv[c] + rr[c]);
            lt[1 + py][1 + 4 * bx + c] = (uint8_t)rec;
            const int e = x[c] + pv[c] - rec;
            sse += (vis && x0 + 4 * bx + c < g.width) ? (uint32_t)(e * e) : 0u;
        }
        if (r == 0) m.nz_luma[by * 4 + bx] = (uint8_t)(luma_ac ? nz : 0);
        cbp_l = luma_ac ? 15 : 0;
        wave_lds_sync();
    }
    if (lane == 0) m.cbp = (uint8_t)cbp_l;  // chroma bits merged at the end of the row
}

// Chroma of one intra macroblock, row layout on lanes 0..31 (lane 4 (comp * 4 + blk) + r).
// cs: the MB's source chroma (8 rows x 4 dwords of interleaved Cb/Cr).
__device__ void intra_chroma_mb(const Geometry& g, int chroma_qp_offset, const MbFields& f, const uint32_t* cs,
                                MbInfo& m, int16_t* __restrict__ mc, int mbx, int mby, const Avail& av,
                                uint8_t (*ct)[9][kCT], int* cdc, int lane, uint32_t& sse_u, uint32_t& sse_v) {
    const int xc0 = mbx * 8, yc0 = mby * 8;
    const int qpc = chroma_qp(f.qp, chroma_qp_offset);
    const QpTab T = qp_tab(qpc);
    const int r = lane & 3, cbk = (lane >> 2) & 7, comp = cbk >> 2, cb = cbk & 3, bx = cb & 1, by = cb >> 1;
    const int py = 4 * by + r;
    const bool clane = lane < 32;
    int pv[4] = {0, 0, 0, 0}, x[4] = {0, 0, 0, 0}, z[4] = {0, 0, 0, 0}, nz = 0;
    if (clane) {
        const NbMb n = nbmb_from_plane(&ct[comp][1][1], kCT, 0, 0, 8, 1, 0, av.left, av.top, av.topleft);
        const PredMb p = prep_chroma(f.chroma_mode, n);
        // samples 4bx .. 4bx+3 of this plane = bytes 8bx + 2c + comp of the interleaved row
        const uint32_t w0 = cs[py * 4 + 2 * bx], w1 = cs[py * 4 + 2 * bx + 1];
        int y[4];
        predmb_row<true>(p, n, 4 * bx, py, pv);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t w = c < 2 ? w0 : w1;
            x[c] = (int)((w >> (8 * (2 * (c & 1) + comp))) & 0xff) - pv[c];
        }
        fdct_row(x, r, y);
        if (r == 0) cdc[comp * 4 + cb] = y[0];
        nz = quad_sum(quant_row_i(y, r, T, 1, z));
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (r * 4 + c > 0) mc[kCoefChromaAc + (comp * 4 + cb) * 16 + zz_inv(r * 4 + c)] = (int16_t)z[c];
        if (r == 0) (comp ? m.nz_cr : m.nz_cb)[cb] = (uint8_t)nz;
    }
    wave_lds_sync();
    int ndc = 0;
    if (lane == 0 || lane == 16) {
        const int cp = lane >> 4;
        int in[4], zd[4], dq[4];
        for (int i = 0; i < 4; ++i) in[i] = cdc[cp * 4 + i];
        ndc = quant_dc_chroma(in, zd, qpc, true);
        for (int i = 0; i < 4; ++i) mc[kCoefChromaDc + cp * 4 + i] = (int16_t)zd[i];
        dequant_dc_chroma(zd, dq, qpc);
        for (int i = 0; i < 4; ++i) cdc[cp * 4 + i] = dq[i];
    }
    wave_lds_sync();
    const bool any_ac = __ballot(clane && nz > 0) != 0, any_dc = __ballot(ndc > 0) != 0;
    if (clane) {
        int d[4], rr[4];
        dequant_row_t(z, r, T, d);
        if (r == 0) d[0] = cdc[comp * 4 + cb];
        idct_row(d, r, rr);
        uint32_t s = 0;
        const bool vis = 2 * (yc0 + py) < g.height;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int xc = xc0 + 4 * bx + c;
            const int rec = clip255(pv[c] + rr[c]);
            const int e = x[c] + pv[c] - rec;
            s += (vis && 2 * xc < g.width) ? (uint32_t)(e * e) : 0u;
            ct[comp][1 + py][1 + 4 * bx + c] = (uint8_t)rec;
        }
        if (comp)
            sse_v += s;
        else
            sse_u += s;
    }
    if (lane == 0) m.cbp_c = (uint8_t)(any_ac ? 2 : (any_dc ? 1 : 0));
    wave_lds_sync();
}


// IDR reconstruction: one workgroup per (slice, plane) -- every MB row of the slice is one wave
// of the workgroup (idr_slice_rows() <= 8), luma and chroma are separate workgroups (the two
// planes' intra predictions are independent).  The diagonal wavefront's row-to-row hand-off
// stays inside the CU: a row publishes each macroblock's bottom sample line into an LDS line
// buffer and then its progress counter; the row below waits on that counter (luma: the MB
// above-right, chroma: the MB above).  LDS operations of one wave complete in issue order,
// so a reader that sees the counter sees the line.  The cross-CU version of this hand-off
// (tagged L2-bypassing line words between per-row workgroups) spent most of its time waiting
// for the stores to become visible (profiles/r02_idr).
struct ChromaWaveTiles {
    uint8_t ct[2][9][kCT];  // chroma tiles (Cb, Cr): row 0 = top neighbours, column 0 = left neighbours
    uint32_t src[64];       // source of the current MB (8 rows x 16 interleaved bytes, lanes 0..31)
    int dc[16];             // chroma DC scratch
};

// The chroma rows of the slice, one macroblock at a time.
__device__ __forceinline__ void intra_chroma_rows(const Geometry& g, const FrameState* __restrict__ fs,
                                                  const uint8_t* __restrict__ src_uv, MbInfo* __restrict__ mbs,
                                                  int16_t* __restrict__ coef, uint8_t* s_line,
                                                  ChromaWaveTiles* tiles, int* prog) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slice_rows = fs->slice_rows, cqp_off = fs->chroma_qp_offset;
    uint8_t* const rec_uv = fs->rec_uv;
    const int mby = blockIdx.x * slice_rows + wave;
    const bool active = mby < g.mb_h;  // the last slice may be shorter (whole waves)
    if (!active) return;  // no workgroup barriers below
    ChromaWaveTiles& T = tiles[wave];
    uint8_t* my_line = s_line + (size_t)wave * g.coded_w;
    const uint8_t* up_line = s_line + (size_t)(wave > 0 ? wave - 1 : 0) * g.coded_w;
    uint32_t sse_a = 0, sse_b = 0;  // U, V
    // software pipeline: the next MB's source dword and fields load while this one is coded
    auto fetch_src = [&](int mbx) -> uint32_t {
        if (mbx >= g.mb_w) return 0u;
        const int r = lane >> 2, c4 = (lane & 3) * 4;
        if (lane >= 32) return 0u;
        return *reinterpret_cast<const uint32_t*>(src_uv + (size_t)(mby * 8 + r) * g.pitch + mbx * 16 + c4);
    };
    uint32_t nsrc = fetch_src(0);
    MbFields nf = load_fields(&mbs[mby * g.mb_w]);
#ifdef MX_IDR_TIMING
    const unsigned long long t_start = wall_clock64();
#endif
    for (int mbx = 0; mbx < g.mb_w; ++mbx) {
        const int mbi = mby * g.mb_w + mbx;
        MbInfo& m = mbs[mbi];
        const MbFields f = nf;
        T.src[lane] = nsrc;
        nsrc = fetch_src(mbx + 1);
        nf = load_fields(&mbs[mby * g.mb_w + (mbx + 1 < g.mb_w ? mbx + 1 : mbx)]);
        const Avail av = mb_avail(g, mbx, mby, slice_rows);
        int16_t* mc = coef + (size_t)mbi * kCoefStride;
        if (av.top) {  // wait for the row above (uniform)
            const int need = mbx + 1;
            while (__hip_atomic_load(&prog[wave - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < need)
                __builtin_amdgcn_s_sleep(1);
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
        }
        {
            const int xc0 = mbx * 8, yc0 = mby * 8;
            uint8_t keep = 0;
            if (lane < 16) keep = T.ct[lane >> 3][1 + (lane & 7)][8];
            // top: lanes 16..33 -> (comp, cx 0..8 = x -1..7), byte 2*(xc0-1+cx)+comp of the line
            const int k = lane - 16, comp_t = k >= 9 ? 1 : 0, cx = k - 9 * comp_t;
            const int x = 2 * (xc0 - 1 + cx) + comp_t;
            const bool need = lane >= 16 && lane < 34 && (cx == 0 ? av.topleft : av.top);
            const uint8_t top = need ? up_line[x] : 0;
            wave_lds_sync();
            if (lane < 16)
                T.ct[lane >> 3][1 + (lane & 7)][0] = av.left ? keep : 0;
            else if (lane < 34)
                T.ct[comp_t][0][cx] = top;
            wave_lds_sync();
            intra_chroma_mb(g, cqp_off, f, T.src, m, mc, mbx, mby, av, T.ct, T.dc, lane, sse_a, sse_b);
            if (lane < 32) {  // 8 rows x 16 interleaved bytes, one dword (2 samples x 2 planes) per lane
                const int r = lane >> 2, c2 = (lane & 3) * 2;
                const uint32_t v = (uint32_t)T.ct[0][1 + r][1 + c2] | ((uint32_t)T.ct[1][1 + r][1 + c2] << 8) |
                                   ((uint32_t)T.ct[0][1 + r][2 + c2] << 16) | ((uint32_t)T.ct[1][1 + r][2 + c2] << 24);
                *reinterpret_cast<uint32_t*>(rec_uv + (size_t)(yc0 + r) * g.pitch + 2 * (xc0 + c2)) = v;
                if (r == 7) *reinterpret_cast<uint32_t*>(my_line + 2 * (xc0 + c2)) = v;
            }
        }
        // publish: the line stores above were issued first, and LDS completes them in order
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        if (lane == 0) __hip_atomic_store(&prog[wave], mbx + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
#ifdef MX_IDR_TIMING
    if (lane == 0)
        printf("MXIDR plane 1 slice %d row %d wall_ticks %llu\n", (int)blockIdx.x, wave, wall_clock64() - t_start);
#endif
    // distortion of the row (one partial per row and channel)
    unsigned long long a = sse_a, b = sse_b;
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    if (lane == 0) {
        fs->sse_part[1 * kSsePartStride + mby] = a;
        fs->sse_part[2 * kSsePartStride + mby] = b;
    }
}

// Luma rows with consecutive Intra4x4 macroblocks pipelined: block (bx, by) of the k-th MB of
// a run of Intra4x4 MBs runs at step 4k + bx + 2by.  Its left neighbours (block (3, by) of
// MB k-1, step 4k - 1 + 2by) and top-left are done a step earlier, and the predecessor copies
// each finished right-column block into the successor's tile; so up to three MBs are in
// flight (one quad pair each, lanes 8j .. 8j+7 for tile slot j = mbx % 3) and a run of n
// such MBs takes 4n + 6 dependent steps instead of 10n.  Intra16x16 MBs (the whole MB's DC
// transform couples all blocks) are coded alone between runs.  The IDR picture QP is
// uniform (k_intra_analyze), so one quantiser table serves every MB in flight.
struct LumaPipeTiles {
    uint8_t lt[3][17][kLT];  // tile slot mbx % 3: row 0 = top neighbours, column 0 = left neighbours
    uint32_t src[3][64];     // the slot MB's source (16 rows x 4 dwords)
    int dc[16];              // Intra16x16 DC scratch
};

__device__ __forceinline__ void intra_luma_rows_pl(const Geometry& g, const FrameState* __restrict__ fs,
                                                   const uint8_t* __restrict__ src_y, MbInfo* __restrict__ mbs,
                                                   int16_t* __restrict__ coef, uint8_t* s_line, LumaPipeTiles* tiles,
                                                   int* prog) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slice_rows = fs->slice_rows;
    uint8_t* const rec_y = fs->rec_y;
    const int mby = blockIdx.x * slice_rows + wave;
    if (mby >= g.mb_h) return;  // the last slice may be shorter (whole waves); no barriers below
    LumaPipeTiles& P = tiles[wave];
    uint8_t* my_line = s_line + (size_t)wave * g.coded_w;
    const uint8_t* up_line = s_line + (size_t)(wave > 0 ? wave - 1 : 0) * g.coded_w;
    const int y0 = mby * 16;
    const QpTab T = qp_tab(fs->qp);
    uint32_t sse_a = 0, sse_m = 0;
    auto fetch_src = [&](int mbx) -> uint32_t {
        if (mbx >= g.mb_w) return 0u;
        const int r = lane >> 2, c4 = (lane & 3) * 4;
        return *reinterpret_cast<const uint32_t*>(src_y + (size_t)(y0 + r) * g.pitch + mbx * 16 + c4);
    };
    uint32_t nsrc = fetch_src(0);
    MbFields nf = load_fields(&mbs[mby * g.mb_w]);
    // stage MB x into its slot: source, top neighbours (after the row above published them) and,
    // if `left`, the left column from the completed previous MB's slot
    auto stage = [&](int x, bool left) {
        const int j = x % 3;
        P.src[j][lane] = nsrc;
        nsrc = fetch_src(x + 1);
        const Avail av = mb_avail(g, x, mby, slice_rows);
        if (av.top) {
            const int need = av.topright ? x + 2 : x + 1;
            while (__hip_atomic_load(&prog[wave - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < need)
                __builtin_amdgcn_s_sleep(1);
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
        }
        const bool need = lane < 21 && (lane == 0 ? av.topleft : (lane <= 16 ? av.top : av.topright));
        const uint8_t top = need ? up_line[x * 16 - 1 + lane] : 0;
        uint8_t lft = 0;
        if (left && lane < 16 && av.left) lft = P.lt[(x + 2) % 3][1 + lane][16];
        wave_lds_sync();
        if (lane < 21) P.lt[j][0][lane] = top;
        if (left && lane < 16) P.lt[j][1 + lane][0] = lft;
        wave_lds_sync();
    };
    // MB x is complete: tile -> reconstruction, bottom line -> LDS, then publish it
    auto finish = [&](int x) {
        const int j = x % 3, x0 = x * 16;
        const int r = lane >> 2, c4 = (lane & 3) * 4;
        const uint32_t v = (uint32_t)P.lt[j][1 + r][1 + c4] | ((uint32_t)P.lt[j][1 + r][2 + c4] << 8) |
                           ((uint32_t)P.lt[j][1 + r][3 + c4] << 16) | ((uint32_t)P.lt[j][1 + r][4 + c4] << 24);
        *reinterpret_cast<uint32_t*>(rec_y + (size_t)(y0 + r) * g.pitch + x0 + c4) = v;
        if (r == 15) *reinterpret_cast<uint32_t*>(my_line + x0 + c4) = v;
        __atomic_signal_fence(__ATOMIC_SEQ_CST);  // LDS completes the line stores before the counter
        if (lane == 0) __hip_atomic_store(&prog[wave], x + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
#ifdef MX_IDR_TIMING
    const unsigned long long t_start = wall_clock64();
#endif
    int next = 0;  // next MB to start
    while (next < g.mb_w) {
        if (nf.type != kMbI4x4) {  // Intra16x16: alone
            const int x = next;
            const MbFields f = nf;
            nf = load_fields(&mbs[mby * g.mb_w + (x + 1 < g.mb_w ? x + 1 : x)]);
            stage(x, true);
            const int j = x % 3, mbi = mby * g.mb_w + x;
            uint32_t sse_mb = 0;
            intra_luma_mb(g, f, P.src[j], mbs[mbi], coef + (size_t)mbi * kCoefStride, x, mby,
                          mb_avail(g, x, mby, slice_rows), P.lt[j], P.dc, lane, sse_mb);
            sse_a += sse_mb;
            if (mb_unmasked(fs, x, mby)) sse_m += sse_mb;
            finish(x);
            ++next;
            continue;
        }
        // a run of Intra4x4 MBs from `base`; MB base + k starts at step 4k while the run lasts
        const int base = next;
        int started = 0;
        bool open = true;
        uint32_t mlo[3] = {0, 0, 0}, mhi[3] = {0, 0, 0};  // Intra4x4 modes per slot (uniform)
        int cbp[3] = {0, 0, 0};
        int sk[3] = {-16, -16, -16};      // run index k of the MB in each slot (uniform)
        bool um[3] = {false, false, false};  // the slot MB counts towards the masked PSNR
        for (int t = 0;; ++t) {
            if ((t & 3) == 0 && open) {
                if (base + started < g.mb_w && nf.type == kMbI4x4) {
                    const int x = base + started, j = x % 3;
                    const MbFields f = nf;
                    nf = load_fields(&mbs[mby * g.mb_w + (x + 1 < g.mb_w ? x + 1 : x)]);
                    const bool unm = mb_unmasked(fs, x, mby);
#pragma unroll
                    for (int s = 0; s < 3; ++s)
                        if (s == j) {
                            mlo[s] = f.i4lo;
                            mhi[s] = f.i4hi;
                            cbp[s] = 0;
                            sk[s] = started;
                            um[s] = unm;
                        }
                    stage(x, started == 0);  // later MBs get their left column from the predecessor
                    ++started;
                } else {
                    open = false;
                }
            }
            if (!open && t > 4 * (started - 1) + 9) break;
            // this lane's MB (slot j = lane / 8, quad group grp) and its local step
            const int j = lane >> 3, grp = (lane >> 2) & 1, r = lane & 3;
            const int k = j == 0 ? sk[0] : (j == 1 ? sk[1] : sk[2]);
            const int sl = t - 4 * k;
            const bool mine = lane < 24 && k >= 0 && sl <= 9;
            const int rb = mine ? i4_step_block(sl, grp) : -1;  // uniform per quad
            int nzb = 0;
            if (rb >= 0) {
                const int x = base + k, mbi = mby * g.mb_w + x;
                const uint32_t lo = j == 0 ? mlo[0] : (j == 1 ? mlo[1] : mlo[2]);
                const uint32_t hi = j == 0 ? mhi[0] : (j == 1 ? mhi[1] : mhi[2]);
                const int mode = (int)(((rb < 8 ? lo : hi) >> (4 * (rb & 7))) & 15u);
                uint32_t e2 = 0;
                nzb = i4_code_block(g, rb, r, mode, T, P.src[j], P.lt[j], coef + (size_t)mbi * kCoefStride, x * 16, y0,
                                    mb_avail(g, x, mby, slice_rows), e2);
                sse_a += e2;
                if (j == 0 ? um[0] : (j == 1 ? um[1] : um[2])) sse_m += e2;
                if (r == 0) mbs[mbi].nz_luma[rb] = (uint8_t)nzb;
            }
            const unsigned long long any = __ballot(rb >= 0 && r == 0 && nzb > 0);
            wave_lds_sync();
            // per slot (uniform): coded-block bits, right-column hand-off, completion
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int ks = sk[s], ss = t - 4 * ks;
                if (ks < 0 || ss > 9) continue;
#pragma unroll
                for (int gq = 0; gq < 2; ++gq)
                    if ((any >> (8 * s + 4 * gq)) & 1ull) cbp[s] |= 1 << (raster_to_blk(i4_step_block(ss, gq)) >> 2);
                if (ss >= 3 && (ss & 1)) {  // block (3, by) done: successor's left column rows 4by .. 4by+3
                    const int by = (ss - 3) >> 1, jn = s == 2 ? 0 : s + 1;  // slot of MB base + ks + 1
                    if (lane < 4) P.lt[jn][1 + 4 * by + lane][0] = P.lt[s][1 + 4 * by + lane][16];
                }
                if (ss == 9) {
                    if (lane == 0) mbs[mby * g.mb_w + base + ks].cbp = (uint8_t)cbp[s];
                    finish(base + ks);
                }
            }
            wave_lds_sync();
        }
        next = base + started;
    }
#ifdef MX_IDR_TIMING
    if (lane == 0) printf("MXIDR plane 0 slice %d row %d wall_ticks %llu\n", (int)blockIdx.x, wave, wall_clock64() - t_start);
#endif
    unsigned long long a = sse_a, mm = sse_m;
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        mm += __shfl_xor(mm, o, 64);
    }
    if (lane == 0) {
        fs->sse_part[0 * kSsePartStride + mby] = a;
        fs->sse_part[3 * kSsePartStride + mby] = mm;
    }
}

__global__ __launch_bounds__(512) void k_intra_wave(Geometry g, const FrameState* __restrict__ fs,
                                                     const uint8_t* __restrict__ src_y,
                                                     const uint8_t* __restrict__ src_uv, MbInfo* __restrict__ mbs,
                                                     int16_t* __restrict__ coef) {
    // a serial chain on few waves: issue priority over the bulk kernels sharing its SIMDs
    __builtin_amdgcn_s_setprio(3);
    extern __shared__ uint8_t s_line[];  // [slice rows][coded_w]: bottom sample line of every coded MB
    __shared__ ChromaWaveTiles tiles[8];    // chroma workgroups
    __shared__ LumaPipeTiles ltiles[8];     // luma workgroups
    __shared__ int prog[8];              // macroblocks of the row whose bottom line is in s_line
    if ((threadIdx.x & 63) == 0) prog[threadIdx.x >> 6] = 0;
    __syncthreads();
    if (blockIdx.y == 0)
        intra_luma_rows_pl(g, fs, src_y, mbs, coef, s_line, ltiles, prog);
    else
        intra_chroma_rows(g, fs, src_uv, mbs, coef, s_line, tiles, prog);
}

// IDR: luma and chroma coded bits merged into the MB's cbp once both planes are done.
__global__ __launch_bounds__(256) void k_intra_cbp(Geometry g, MbInfo* __restrict__ mbs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.mb_w * g.mb_h) return;
    MbInfo& m = mbs[i];
    m.cbp = (uint8_t)((m.cbp & 15) | (m.cbp_c << 4));
}

// Intra macroblocks of P pictures (independent by construction, see intra_selected()): one
// workgroup per macroblock, luma on wave 0 and chroma on wave 1, neighbours straight from the
// final inter reconstruction, coded by the same routines as k_intra_wave.  The distortion
// delta against the MB's inter distortion goes into its row's partial (atomic, few MBs).
__device__ void intra_p_mb(const Geometry& g, const FrameState* __restrict__ fs, const uint8_t* __restrict__ src_y,
                           const uint8_t* __restrict__ src_uv, MbInfo* __restrict__ mbs, int16_t* __restrict__ coef,
                           const int32_t* __restrict__ gain, const uint32_t* __restrict__ mb_sse, int mbi) {
    __shared__ uint8_t lt[17][kLT];
    __shared__ uint8_t ct[2][9][kCT];
    __shared__ uint32_t ls[64];
    __shared__ uint32_t cs[32];
    __shared__ int ldc[16], cdc[8];
    const int mbx = mbi % g.mb_w, mby = mbi / g.mb_w;
    if (!intra_selected(gain, g.mb_w, g.mb_h, mbx, mby)) return;  // uniform over the workgroup
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    MbInfo& m = mbs[mbi];
    MbFields f = load_fields(&m);
    f.type = m.itype;
    f.qp = fs->qp;
    const Avail av = mb_avail(g, mbx, mby, fs->slice_rows);
    int16_t* mc = coef + (size_t)mbi * kCoefStride;
    uint32_t s0 = 0, s1 = 0;
    __syncthreads();  // every wave has read the MB fields before they are overwritten
    if (threadIdx.x == 0) {
        m.type = (uint8_t)f.type;
        m.qp = (uint8_t)f.qp;
        m.mvx = 0;
        m.mvy = 0;
    }
    if (wave == 0) {
        const int x0 = mbx * 16, y0 = mby * 16;
        {
            const int r = lane >> 2, c4 = (lane & 3) * 4;
            ls[lane] = *reinterpret_cast<const uint32_t*>(src_y + (size_t)(y0 + r) * g.pitch + x0 + c4);
        }
        if (lane < 16) lt[1 + lane][0] = av.left ? fs->rec_y[(y0 + lane) * g.pitch + x0 - 1] : 0;
        if (lane < 21) {
            const bool ok = lane == 0 ? av.topleft : (lane <= 16 ? av.top : av.topright);
            lt[0][lane] = ok ? fs->rec_y[(y0 - 1) * g.pitch + x0 - 1 + lane] : 0;
        }
        wave_lds_sync();
        intra_luma_mb(g, f, ls, m, mc, mbx, mby, av, lt, ldc, lane, s0);
        const int r = lane >> 2, c4 = (lane & 3) * 4;
        const uint32_t v = (uint32_t)lt[1 + r][1 + c4] | ((uint32_t)lt[1 + r][2 + c4] << 8) |
                           ((uint32_t)lt[1 + r][3 + c4] << 16) | ((uint32_t)lt[1 + r][4 + c4] << 24);
        *reinterpret_cast<uint32_t*>(fs->rec_y + (y0 + r) * g.pitch + x0 + c4) = v;
    } else {
        const int xc0 = mbx * 8, yc0 = mby * 8;
        if (lane < 32) {
            const int r = lane >> 2, c4 = (lane & 3) * 4;
            cs[lane] = *reinterpret_cast<const uint32_t*>(src_uv + (size_t)(yc0 + r) * g.pitch + mbx * 16 + c4);
        }
        if (lane < 16) {
            const int comp = lane >> 3, r = lane & 7;
            ct[comp][1 + r][0] = av.left ? fs->rec_uv[(yc0 + r) * g.pitch + 2 * (xc0 - 1) + comp] : 0;
        } else if (lane < 34) {
            const int k = lane - 16, comp = k / 9, cx = k - comp * 9;
            const bool ok = cx == 0 ? av.topleft : av.top;
            ct[comp][0][cx] = ok ? fs->rec_uv[(yc0 - 1) * g.pitch + 2 * (xc0 - 1 + cx) + comp] : 0;
        }
        wave_lds_sync();
        intra_chroma_mb(g, fs->chroma_qp_offset, f, cs, m, mc, mbx, mby, av, ct, cdc, lane, s0, s1);
        if (lane < 32) {
            const int r = lane >> 2, c2 = (lane & 3) * 2;
            const uint32_t v = (uint32_t)ct[0][1 + r][1 + c2] | ((uint32_t)ct[1][1 + r][1 + c2] << 8) |
                               ((uint32_t)ct[0][1 + r][2 + c2] << 16) | ((uint32_t)ct[1][1 + r][2 + c2] << 24);
            *reinterpret_cast<uint32_t*>(fs->rec_uv + (yc0 + r) * g.pitch + 2 * (xc0 + c2)) = v;
        }
    }
    unsigned long long a = s0, b = s1;
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    __syncthreads();  // both waves done: merge the chroma cbp
    const int nmb = g.mb_w * g.mb_h;
    const int slot = mby;  // the row's delta (k_intra_analyze zeroed it): k_scan_rows adds it to the inter sums
    if (lane == 0) {
        if (wave == 0) {
            m.cbp = (uint8_t)((m.cbp & 15) | (m.cbp_c << 4));
            atomicAdd(&fs->sse_part[slot], a - mb_sse[mbi]);
            if (mb_unmasked(fs, mbx, mby)) atomicAdd(&fs->sse_part[3 * kSsePartStride + slot], a - mb_sse[mbi]);
        } else {
            atomicAdd(&fs->sse_part[kSsePartStride + slot], a - mb_sse[nmb + mbi]);
            atomicAdd(&fs->sse_part[2 * kSsePartStride + slot], b - mb_sse[2 * nmb + mbi]);
        }
    }
}

__global__ __launch_bounds__(128) void k_intra_p(Geometry g, const FrameState* __restrict__ fs,
                                                 const uint8_t* __restrict__ src_y, const uint8_t* __restrict__ src_uv,
                                                 MbInfo* __restrict__ mbs, int16_t* __restrict__ coef,
                                                 const int32_t* __restrict__ gain, const uint32_t* __restrict__ mb_sse,
                                                 const int* __restrict__ wave_prog, const int* __restrict__ cand) {
    // the candidates (positive gain) listed by k_intra_analyze; a fixed grid walks the list
    const int ncand = wave_prog[1];
    for (int k = blockIdx.x; k < ncand; k += gridDim.x) intra_p_mb(g, fs, src_y, src_uv, mbs, coef, gain, mb_sse, cand[k]);
}

// ------------------------------------------------------------------ CAVLC
__device__ __forceinline__ uint32_t mask_bits(int n) { return n >= 32 ? 0xffffffffu : ((1u << n) - 1); }

// OR the overlap of segment [s0, s0+len) with output word [W0, W0+32) into acc; getbits
// returns `n` segment-relative bits starting at `a`.
template <class F>
__device__ __forceinline__ void overlap(uint32_t& acc, uint32_t W0, uint32_t s0, uint32_t len, F getbits) {
    const uint32_t lo = max(W0, s0), hi = min(W0 + 32, s0 + len);
    if (lo >= hi) return;
    const int n = (int)(hi - lo);
    const uint32_t bits = getbits(lo - s0, n) & mask_bits(n);
    acc |= bits << (W0 + 32 - hi);
}

// One wave per MB, one CAVLC "role" per lane.  Single coding pass: each role writes its bits
// MSB-first into a private LDS buffer; a wave prefix sum of the bit counts places the roles;
// then each lane assembles whole output words of the MB slot from the (at most a few) role
// buffers overlapping them and stores them straight to the global slot.
constexpr int kRoleWords = 24;  // worst-case CAVLC 4x4 block ~630 bits
__device__ __forceinline__ uint32_t role_get(const uint32_t* buf, uint32_t b, int n) {
    const uint32_t wi = b >> 5, sh = b & 31;
    const uint64_t hi = ((uint64_t)buf[wi] << 32) | (wi + 1 < (uint32_t)kRoleWords ? buf[wi + 1] : 0u);
    return (uint32_t)((hi << sh) >> (64 - n));
}

// Two macroblocks per wave (one per 32-lane half): the 28 roles of an MB fill a half, so a
// wave no longer idles 36 of its 64 lanes; the prefix sum, ballots and word assembly are
// segmented per half.
constexpr int kCavlcMbPerBlock = 8;
// kQuad: the picture may hold P_8x8 macroblocks (EncoderConfig::partitions 2).  A template kernel: behind a
// shared device function k_cavlc<false> did not compile to the instructions k_cavlc had.
template <bool kQuad>
__global__ __launch_bounds__(256) void k_cavlc(Geometry g, const FrameState* __restrict__ fs, MbInfo* __restrict__ mbs,
                                               const int16_t* __restrict__ coef, uint32_t* __restrict__ slot,
                                               uint32_t* __restrict__ slot_bits) {
    static_assert(kNumRoles < 32, "the roles of one MB (plus the total slot) must fit a half-wave");
    __shared__ uint32_t rbuf[kCavlcMbPerBlock][kNumRoles][kRoleWords];
    __shared__ uint32_t roff[kCavlcMbPerBlock][kNumRoles + 1];
    __shared__ __attribute__((aligned(16))) int16_t cbuf[kCavlcMbPerBlock][kCoefStride];
    __shared__ MbInfo nbuf[kCavlcMbPerBlock][5];  // self, left, top, top-right, top-left
    static_assert(sizeof(MbInfo) % 4 == 0, "MbInfo copied as dwords");
    const int hw = (threadIdx.x >> 5) & 1, lane = threadIdx.x & 31;  // hw: half of the wave; lane = role
    const int wave = threadIdx.x >> 5;                                   // MB slot in the block (half-wave)
    const int nmb = g.mb_w * g.mb_h;
    const int mbi = blockIdx.x * kCavlcMbPerBlock + wave;
    if (mbi >= nmb) return;  // a whole half exits; only half-local shuffles below, no workgroup barrier
    const int mbx = mbi % g.mb_w, mby = mbi / g.mb_w;
    const Avail av = mb_avail(g, mbx, mby, fs->slice_rows);
    // the MB's and its available neighbours' MbInfo into LDS (12 dwords each, one load round):
    // the role coders read their fields in data-dependent order, from global memory that was
    // a chain of L2 round trips
    {
        const int src[5] = {mbi, mbi - 1, mbi - g.mb_w, mbi - g.mb_w + 1, mbi - g.mb_w - 1};
        const bool ok[5] = {true, av.left, av.top, av.topright, av.topleft};
        constexpr int kW = (int)(sizeof(MbInfo) / 4);
        for (int q = lane; q < 5 * kW; q += 32) {
            const int k = q / kW, d = q - k * kW;
            if (ok[k]) reinterpret_cast<uint32_t*>(&nbuf[wave][k])[d] = reinterpret_cast<const uint32_t*>(&mbs[src[k]])[d];
        }
        wave_lds_sync();
    }
    const MbNbrs nb{&nbuf[wave][0], &nbuf[wave][1], &nbuf[wave][2], &nbuf[wave][3], &nbuf[wave][4]};
    const MbInfo& m = nbuf[wave][0];
    const int16_t* mc = coef + (size_t)mbi * kCoefStride;

    // motion vector prediction + P_Skip decision (every lane computes the same values)
    int mvd[kQuad ? 8 : 4];
    const bool skip = decide_skip<kQuad>(nb, av, mvd);
    // mb_qp_delta: QP predictor = QP of the previous MB in the slice that carried one (a P
    // macroblock with residual); skipped / residual-free MBs inherit it.  Half-wave-parallel
    // backward search (the ballot holds active lanes only; this half's bits are taken), 512 MBs
    // per step: each lane tests 16 (independent loads, one latency per step) -- static desktop
    // areas are long skip runs, and at 128 MBs per step the dependent steps through them were
    // ~7 us of k_cavlc (a separate scan kernel cost more than it saved: profiles/r03_h264).
    // I slices: every MB is at the slice QP.
    int dqp = 0;
    if (!skip && !fs->idr && carries_dqp(m)) {
        const int per_slice = fs->slice_rows * g.mb_w, first = (mbi / per_slice) * per_slice;
        int pred = fs->qp;
        bool found = false;
        constexpr int kPer = 16;
        for (int j0 = mbi - 1; j0 >= first && !found; j0 -= 32 * kPer) {
            int qv[kPer];
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                const int j = j0 - 32 * k - lane;
                qv[k] = -1;
                if (j >= first) {
                    const MbInfo& mj = mbs[j];
                    if (carries_dqp(mj)) qv[k] = mj.qp;
                }
            }
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                const unsigned long long bal = __ballot(qv[k] >= 0);
                const uint32_t hb = (uint32_t)(bal >> (32 * hw));
                const int q = __shfl(qv[k], hb ? (int)(__ffs(hb) - 1) : 0, 32);
                if (!found && hb) {
                    pred = q;
                    found = true;
                }
            }
        }
        dqp = qp_delta(m.qp, pred);
    }
    // the MB's coefficients into LDS first (one 16-byte load per lane and pass): the CAVLC
    // scans re-read them in data-dependent loops, which from global memory were chains of
    // dependent L2 round trips
    if (!skip) {
        const uint4* src = reinterpret_cast<const uint4*>(mc);
        uint4* dst = reinterpret_cast<uint4*>(cbuf[wave]);
        for (int q = lane; q < kCoefStride / 8; q += 32) dst[q] = src[q];
    }
    wave_lds_sync();
    uint32_t bits = 0;
    if (!skip && lane < kNumRoles) {
        BitWriter w;
        w.init(rbuf[wave][lane]);
        code_role<kQuad>(w, lane, g, fs->idr, nb, cbuf[wave], av, mvd, dqp);
        w.flush();
        bits = w.bits;
    }
    // exclusive prefix sum of bits over the half's lanes -> role offsets in the MB slot
    // (DPP: shift-add scan within rows of 16, then row_bcast:15 into the odd rows -- rows 0-1 and
    // 2-3 are the two halves -- instead of five lane-shuffle round trips)
    uint32_t incl = bits;
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x111, 0xF, 0xF, false);  // row_shr:1
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x112, 0xF, 0xF, false);  // row_shr:2
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x114, 0xF, 0xF, false);  // row_shr:4
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x118, 0xF, 0xF, false);  // row_shr:8
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x142, 0xA, 0xF, false);  // row_bcast:15
    const uint32_t total = __shfl(incl, 31, 32);
    if (lane < kNumRoles) roff[wave][lane] = incl - bits;
    if (lane == kNumRoles) roff[wave][kNumRoles] = total;
    wave_lds_sync();
    const bool fits = total <= kSlotWords * 32u;
    if (!skip && fits) {
        const uint32_t nwords = (total + 31) >> 5;
        uint32_t* dst = slot + (size_t)mbi * kSlotWords;
        for (uint32_t wi = lane; wi < nwords; wi += 32) {
            const uint32_t W0 = wi * 32;
            // first role ending after W0 (roles are contiguous and in lane order)
            int r = 0;
            while (r < kNumRoles - 1 && roff[wave][r + 1] <= W0) ++r;
            uint32_t acc = 0;
            for (; r < kNumRoles; ++r) {
                const uint32_t o = roff[wave][r], len = roff[wave][r + 1] - o;
                if (o >= W0 + 32) break;
                if (len == 0) continue;
                overlap(acc, W0, o, len, [&](uint32_t x, int n) { return role_get(rbuf[wave][r], x, n); });
            }
            dst[wi] = acc;
        }
    }
    if (lane == 0) {
        slot_bits[mbi] = skip ? 0u : (fits ? total : 0xffffffffu);
        mbs[mbi].skip = skip ? 1 : 0;
    }
}

// ------------------------------------------------------------------ scan (two passes, one workgroup per MB row)
// The bitstream layout needs, for every coded MB, its unit's absolute bit offset: unit bits =
// ue(skip run) + MB bits, slices byte-aligned behind their headers.  Pass 1 (k_scan_rows)
// summarises each MB row; pass 2 (k_scan_out) has every workgroup rebuild the row / slice
// prefixes from those summaries (a few hundred values) and lay out its own row.  Both passes
// spread the work over mb_h workgroups (a single-workgroup scan was latency bound at ~25 us).
constexpr int kScanThreads = 256;
constexpr int kScanRowPer = 2;   // MBs per thread in a row: mb_w <= 512
constexpr int kScanMaxRows = 512;

__device__ __forceinline__ uint32_t blk_excl_sum(uint32_t v, uint32_t* wbuf, uint32_t* total) {
    return blk_excl_scan<kScanThreads, uint32_t>(v, 0u, [](uint32_t a, uint32_t b) { return a + b; }, wbuf, total);
}
__device__ __forceinline__ int blk_excl_max(int v, int init, int* wbuf, int* total) {
    return blk_excl_scan<kScanThreads, int>(v, init, [](int a, int b) { return max(a, b); }, wbuf, total);
}

__device__ __forceinline__ SliceParams slice_params(const FrameState* fs, int s, int mb_w) {
    return make_slice_params(s * fs->slice_rows * mb_w, fs->idr, fs->frame_num, fs->log2_max_frame_num,
                             fs->idr_pic_id, fs->qp - fs->pic_init_qp, fs->deblock_off);
}

// Pass 1, row r: {first coded MB or -1, last coded MB or -1, coded count | overflow << 31,
// unit bits of the row excluding the skip-run prefix of its first coded MB (that run depends
// on earlier rows)}; and this row's share of the distortion partials.
// slot_bits[i]: 0 = P_Skip, 0xffffffff = slot overflow, else coded MB bits (>= 1).
// (kQuad: as k_cavlc -- the adaptive filter's class counts have a rule for P_8x8 macroblocks)
template <bool kQuad>
__global__ __launch_bounds__(kScanThreads) void k_scan_rows(Geometry g, const FrameState* __restrict__ fs,
                                                            const uint32_t* __restrict__ slot_bits,
                                                            uint4* __restrict__ row_agg,
                                                            unsigned long long* __restrict__ row_sse,
                                                            const MbInfo* __restrict__ mbs, uint32_t* __restrict__ db_cnt,
                                                            const uint32_t* __restrict__ mb_sse) {
    __shared__ int wi[kScanThreads / 64];
    __shared__ uint32_t wu[kScanThreads / 64];
    const int t = threadIdx.x, r = blockIdx.x, base = r * g.mb_w;
    const bool idr = fs->idr != 0;
    // this row's distortion: its partial (k_intra_wave's in an I picture, k_db_sse's when the in-loop
    // filter is on), or the per-macroblock sums the P coder left in mb_sse plus, with intra_in_p,
    // k_intra_p's delta of the row
    const int nmb = g.mb_w * g.mb_h;
    const bool per_mb = !idr && fs->deblock_off;
    unsigned long long acc[4] = {0, 0, 0, 0};
    if (per_mb) {
        for (int j = t; j < g.mb_w; j += kScanThreads) {
            const uint32_t sy = mb_sse[base + j];
            acc[0] += sy;
            acc[1] += mb_sse[nmb + base + j];
            acc[2] += mb_sse[2 * nmb + base + j];
            acc[3] += mb_unmasked(fs, j, r) ? sy : 0u;
        }
    }
    if (t == 0 && (!per_mb || fs->intra_in_p))
        for (int c = 0; c < 4; ++c) acc[c] += fs->sse_part[c * kSsePartStride + r];
    uint32_t b[kScanRowPer];
    int last = -1, first = 0x7fffffff;
    uint32_t ncoded = 0, over = 0;
#pragma unroll
    for (int k = 0; k < kScanRowPer; ++k) {
        const int j = t * kScanRowPer + k;
        b[k] = j < g.mb_w ? slot_bits[base + j] : 0u;
        if (b[k] == 0xffffffffu) {
            over = 1;
            b[k] = 1;
        }
        if (b[k]) {
            last = base + j;
            first = min(first, base + j);
            ++ncoded;
        }
    }
    int lastall;
    int prev = blk_excl_max(last, -1, wi, &lastall);  // last coded MB of the row before this thread
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < kScanRowPer; ++k) {
        if (!b[k]) continue;
        const int i = base + t * kScanRowPer + k;
        if (prev >= 0 && !idr) bits += (uint32_t)ue_len((uint32_t)(i - prev - 1));
        bits += b[k];
        prev = i;
    }
    uint32_t tb, tc, to;
    (void)blk_excl_sum(bits, wu, &tb);
    (void)blk_excl_sum(ncoded, wu, &tc);
    (void)blk_excl_sum(over, wu, &to);
    int firstall;
    (void)blk_excl_scan<kScanThreads, int>(first, 0x7fffffff, [](int x, int y) { return min(x, y); }, wi, &firstall);
    if (t == 0)
        row_agg[r] = make_uint4((uint32_t)(lastall >= 0 ? firstall : -1), (uint32_t)lastall,
                                tc | (to ? 0x80000000u : 0u), tb);
    __shared__ unsigned long long red[4][kScanThreads / 64];
    for (int c = 0; c < 4; ++c) {
        unsigned long long v = acc[c];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((t & 63) == 0) red[c][t >> 6] = v;
    }
    __syncthreads();
    if (t < 4) {
        unsigned long long v = 0;
        for (int w = 0; w < kScanThreads / 64; ++w) v += red[t][w];
        row_sse[t * kScanMaxRows + r] = v;
    }
    if (idr || !db_cnt) return;
    // adaptive in-loop filter: this row's temporal-class counts (h264_deblock.h db_auto_count)
    DbAutoCounts ac;
    for (int j = t; j < g.mb_w; j += kScanThreads) db_auto_count<kQuad>(mbs, g.mb_w, base + j, ac);
    uint32_t cv[3] = {ac.coherent, ac.changed, ac.moving};
    __shared__ uint32_t cred[3][kScanThreads / 64];
    for (int c = 0; c < 3; ++c) {
        for (int o = 32; o > 0; o >>= 1) cv[c] += __shfl_xor(cv[c], o);
        if ((t & 63) == 0) cred[c][t >> 6] = cv[c];
    }
    __syncthreads();
    if (t < 3) {
        uint32_t v = 0;
        for (int w = 0; w < kScanThreads / 64; ++w) v += cred[t][w];
        if (v) atomicAdd(&db_cnt[t], v);
    }
}

// Pass 2, row r: row / slice prefixes from all rows' summaries, then this row's units:
// coded_info[rank] = {absolute bit offset, MB index, unit bits, skip run} and the quad -> unit
// table for k_pack (rank of the unit -- or of the slice's first / end unit for header /
// trailer bits -- holding each 128-bit output quad's first bit).  The workgroup of a slice's
// first row writes slice_info; row 0 writes the header and the frame distortion.
__global__ __launch_bounds__(kScanThreads) void k_scan_out(Geometry g, const FrameState* __restrict__ fs,
                                                           const uint32_t* __restrict__ slot_bits,
                                                           const uint4* __restrict__ row_agg,
                                                           const unsigned long long* __restrict__ row_sse,
                                                           uint4* __restrict__ coded_info,
                                                           uint32_t* __restrict__ slice_info, size_t out_bytes,
                                                           OutHeader* __restrict__ hdr,
                                                           uint32_t* __restrict__ quad_unit, uint32_t* __restrict__ db_cnt,
                                                           const int32_t* __restrict__ scroll_hint) {
    __shared__ int s_lbraw[kScanMaxRows + 1];    // last coded MB before row j (any slice), -1 = none
    __shared__ uint32_t s_P[kScanMaxRows + 1];   // unit bits before row j (frame-wide running sum)
    __shared__ uint32_t s_R[kScanMaxRows + 1];   // coded MBs before row j
    __shared__ uint32_t s_soff[kScanThreads + 1], s_sbytes[kScanThreads], s_hbits[kScanThreads];
    __shared__ int wi[kScanThreads / 64];
    __shared__ uint32_t wu[kScanThreads / 64];
    const int t = threadIdx.x, r = blockIdx.x, mb_w = g.mb_w, mb_h = g.mb_h;
    const bool idr = fs->idr != 0;
    const int srows = fs->slice_rows, ns = fs->num_slices;
    // this row's MB bits, loaded up front (independent of the prefix work below)
    const int base = r * mb_w;
    uint32_t b[kScanRowPer];
#pragma unroll
    for (int k = 0; k < kScanRowPer; ++k) {
        const int j = t * kScanRowPer + k;
        b[k] = j < mb_w ? slot_bits[base + j] : 0u;
    }
    // frame distortion (row 0): the per-row sums, reduced by the whole workgroup
    unsigned long long dsum[4] = {0, 0, 0, 0};
    if (r == 0)
        for (int j = t; j < mb_h; j += kScanThreads)
            for (int c = 0; c < 4; ++c) dsum[c] += row_sse[c * kScanMaxRows + j];
    // rows t*2, t*2+1 of the frame per thread (mb_h <= kScanMaxRows)
    uint4 ag[2];
    int lastr = -1;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int j = 2 * t + k;
        ag[k] = j < mb_h ? row_agg[j] : make_uint4(0xffffffffu, 0xffffffffu, 0u, 0u);
        lastr = max(lastr, (int)ag[k].y);
    }
    int dummy, lastframe;
    int lb = blk_excl_max(lastr, -1, wi, &lastframe);
    uint32_t contrib[2], nc[2], over = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int j = 2 * t + k;
        contrib[k] = 0;
        nc[k] = ag[k].z & 0x7fffffffu;
        over |= ag[k].z >> 31;
        if (j < mb_h) {
            s_lbraw[j] = lb;
            const int sfirst = (j / srows) * srows * mb_w;
            const int pv = max(lb, sfirst - 1);
            contrib[k] = ag[k].w;
            if ((int)ag[k].x >= 0 && !idr) contrib[k] += (uint32_t)ue_len((uint32_t)((int)ag[k].x - pv - 1));
        }
        lb = max(lb, (int)ag[k].y);
    }
    uint32_t ptot, rtot, otot;
    uint32_t pex = blk_excl_sum(contrib[0] + contrib[1], wu, &ptot);
    uint32_t rex = blk_excl_sum(nc[0] + nc[1], wu, &rtot);
    (void)blk_excl_sum(over, wu, &otot);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int j = 2 * t + k;
        if (j < mb_h) {
            s_P[j] = pex;
            s_R[j] = rex;
        }
        pex += contrib[k];
        rex += nc[k];
    }
    if (t == 0) {
        s_P[mb_h] = ptot;
        s_R[mb_h] = rtot;
        s_lbraw[mb_h] = lastframe;
    }
    __syncthreads();
    // slice sizes (ns <= kScanThreads: IDR slices are >= mb_h / 16 rows, P pictures one slice)
    uint32_t sbytes = 0, hb = 0;
    if (t < ns) {
        const int fr = t * srows, er = min(fr + srows, mb_h);
        const int sfirst = fr * mb_w, slast = er * mb_w - 1;
        const uint32_t data = s_P[er] - s_P[fr];
        const int lastin = max(s_lbraw[er], sfirst - 1);
        const uint32_t trail = idr ? 0u : (uint32_t)(slast - lastin);
        BitCounter bc;
        bc.init(nullptr);
        write_slice_header(bc, slice_params(fs, t, mb_w));
        hb = bc.bits;
        const uint32_t bits = hb + data + (trail ? ue_len(trail) : 0) + 1;
        sbytes = (bits + 7) >> 3;
    }
    uint32_t total_bytes;
    const uint32_t soff = blk_excl_sum(sbytes, wu, &total_bytes);
    if (t < ns) {
        s_soff[t] = soff;
        s_sbytes[t] = sbytes;
        s_hbits[t] = hb;
    }
    __syncthreads();
    const uint32_t nquads_max = (uint32_t)((out_bytes + 15) / 16);
    auto mark_quads = [&](uint32_t a, uint32_t len, uint32_t rk) {  // quads starting in [a, a + len)
        if (len == 0) return;
        const uint32_t qe = min((a + len - 1) >> 7, nquads_max - 1);
        for (uint32_t q = (a + 127) >> 7; q <= qe; ++q) quad_unit[q] = rk;
    };
    const int s = r / srows, fr = s * srows, er = min(fr + srows, mb_h);
    const uint32_t sbase = s_soff[s] * 8 + s_hbits[s];  // output bit of the slice's first unit
    // slice-level records (the slice's first row)
    if (r == fr && t == 0) {
        const uint32_t data = s_P[er] - s_P[fr];
        const int sfirst = fr * mb_w, slast = er * mb_w - 1;
        const int lastin = max(s_lbraw[er], sfirst - 1);
        const uint32_t trail = idr ? 0u : (uint32_t)(slast - lastin);
        uint32_t* si = slice_info + kSliceInfo * s;
        si[0] = s_hbits[s];
        si[1] = s_soff[s];
        si[2] = s_sbytes[s];
        si[3] = trail;
        si[4] = sbase + data;  // data end (trailer start)
        si[5] = s_P[fr];
        si[6] = s_R[fr];  // coded MBs before the slice
        si[7] = s_R[er];
        if (total_bytes <= out_bytes) {  // header and trailer quads of the slice
            mark_quads(s_soff[s] * 8, s_hbits[s], s_R[fr]);
            const uint32_t dend = sbase + data;
            mark_quads(dend, s_soff[s] * 8 + s_sbytes[s] * 8 - dend, s_R[er]);
        }
    }
    if (r == 0) {
        __shared__ unsigned long long red[4][kScanThreads / 64];
        for (int c = 0; c < 4; ++c) {
            unsigned long long v = dsum[c];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if ((t & 63) == 0) red[c][t >> 6] = v;
        }
        __syncthreads();
        if (t < 4) {
            unsigned long long v = 0;
            for (int w = 0; w < kScanThreads / 64; ++w) v += red[t][w];
            if (t < 3)
                hdr->sse[t] = v;
            else
                hdr->sse_masked = v;
        }
        if (t == 0) {
            const bool over_b = total_bytes > out_bytes;
            hdr->total_bytes = over_b ? 0 : total_bytes;
            hdr->num_slices = ns;
            hdr->overflow = (otot ? 1u : 0u) | (over_b ? 2u : 0u);
            hdr->deblocked = fs->deblock_off ? 0u : 1u;
            hdr->db_coherent = db_cnt ? db_cnt[0] : 0u;
            hdr->db_changed = db_cnt ? db_cnt[1] : 0u;
            hdr->db_moving = db_cnt ? db_cnt[2] : 0u;
            if (db_cnt) db_cnt[0] = db_cnt[1] = db_cnt[2] = 0;  // re-armed for the slot's next frame
            const bool hinted = !fs->idr && scroll_hint;  // the hint k_scroll_decide left for this P picture
            hdr->scroll_dx = (int16_t)(hinted ? scroll_hint[0] : 0);
            hdr->scroll_dy = (int16_t)(hinted ? scroll_hint[1] : 0);
        }
    }
    // this row's units
    const int sfirst = fr * mb_w;
    int last = -1;
    uint32_t ncod = 0;
#pragma unroll
    for (int k = 0; k < kScanRowPer; ++k) {
        const int j = t * kScanRowPer + k;
        if (b[k] == 0xffffffffu) b[k] = 1;
        if (b[k]) {
            last = base + j;
            ++ncod;
        }
    }
    int prev = blk_excl_max(last, max(s_lbraw[r], sfirst - 1), wi, &dummy);
    uint32_t ub[kScanRowPer], run[kScanRowPer], ltot = 0;
#pragma unroll
    for (int k = 0; k < kScanRowPer; ++k) {
        ub[k] = 0;
        run[k] = 0;
        if (!b[k]) continue;
        const int i = base + t * kScanRowPer + k;
        run[k] = (uint32_t)(i - prev - 1);
        ub[k] = (idr ? 0u : (uint32_t)ue_len(run[k])) + b[k];
        ltot += ub[k];
        prev = i;
    }
    uint32_t rowbits, rowcoded;
    uint32_t off = sbase + (s_P[r] - s_P[fr]) + blk_excl_sum(ltot, wu, &rowbits);
    uint32_t rk = s_R[r] + blk_excl_sum(ncod, wu, &rowcoded);
#pragma unroll
    for (int k = 0; k < kScanRowPer; ++k) {
        if (!ub[k]) continue;
        const int i = base + t * kScanRowPer + k;
        coded_info[rk] = make_uint4(off, (uint32_t)i, ub[k], run[k]);
        mark_quads(off, ub[k], rk);
        off += ub[k];
        ++rk;
    }
}

// ------------------------------------------------------------------ pack (gather)
// n bits (1..32) starting at bit b of an MB slot.
__device__ __forceinline__ uint32_t slot_get(const uint32_t* slot, uint32_t b, int n) {
    const uint32_t wi = b >> 5, sh = b & 31;
    const uint64_t hi = ((uint64_t)slot[wi] << 32) | (wi + 1 < (uint32_t)kSlotWords ? slot[wi + 1] : 0u);
    return (uint32_t)((hi << sh) >> (64 - n));
}



// One thread per 32-bit output word, four lanes per 16-byte quad: each lane locates its
// word's first overlapping slice / MB unit (4-ary search over the dense per-rank unit
// records written by k_scan_out), assembles the word from the slice header / MB units / slice
// trailer bits that overlap it, and lane 0 of the quad gathers the four words with lane
// shuffles and writes them with one 16-byte store straight into pinned host memory.
// No atomics, no zero-fill pass, short dependent-load chains (latency-bound kernel).
__device__ void pack_body(const Geometry& g, const FrameState* __restrict__ fs, const uint32_t* __restrict__ slot,
                          const uint4* __restrict__ coded_info, const uint32_t* __restrict__ slice_info,
                          const OutHeader& h, uint8_t* __restrict__ host, const uint32_t* __restrict__ quad_unit);

__global__ __launch_bounds__(256) void k_pack(Geometry g, const FrameState* __restrict__ fs,
                                              const uint32_t* __restrict__ slot,
                                              const uint4* __restrict__ coded_info,
                                              const uint32_t* __restrict__ slice_info,
                                              const OutHeader* __restrict__ hdr, uint8_t* __restrict__ host,
                                              const uint32_t* __restrict__ quad_unit, uint32_t* __restrict__ done) {
    const OutHeader h = *hdr;
    pack_body(g, fs, slot, coded_info, slice_info, h, host, quad_unit);
    // the last workgroup to finish stamps the frame's end time into the host header (the host
    // reads it after the frame's completion event) and re-arms the counter for the next frame
    __syncthreads();
    if (threadIdx.x == 0) {
        // relaxed: only the count matters (the host reads the header after the frame's completion
        // event); acq_rel put an L2 write-back (buffer_wbl2) + invalidate around it in every one of
        // the workgroups
        const uint32_t prev = __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == gridDim.x - 1) {
            reinterpret_cast<OutHeader*>(host)->t_end = wall_clock64();
            __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__device__ void pack_body(const Geometry& g, const FrameState* __restrict__ fs, const uint32_t* __restrict__ slot,
                          const uint4* __restrict__ coded_info, const uint32_t* __restrict__ slice_info,
                          const OutHeader& h, uint8_t* __restrict__ host, const uint32_t* __restrict__ quad_unit) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    if (gid == 0) *reinterpret_cast<OutHeader*>(host) = h;
    uint32_t* hs = reinterpret_cast<uint32_t*>(host + sizeof(OutHeader));
    for (size_t s = gid; s < h.num_slices; s += stride) {
        hs[s] = slice_info[kSliceInfo * s + 1];
        hs[kMaxSlices + s] = slice_info[kSliceInfo * s + 2];
    }
    if (h.overflow) return;
    const bool idr = fs->idr != 0;
    const int ns = (int)h.num_slices;
    const uint32_t nquads = (h.total_bytes + 15) / 16;
    uint4* out = reinterpret_cast<uint4*>(host + kOutPayloadOffset);
    const int sub = threadIdx.x & 3;  // word within the quad
    // all four lanes of a quad iterate together (uniform trip count for the shuffles)
    for (size_t qbase = gid >> 2; qbase < ((nquads + 63) / 64) * 64; qbase += stride >> 2) {
        const bool active = qbase < nquads;
        uint32_t acc = 0;
        if (active) {
            const uint32_t W0 = (uint32_t)qbase * 128 + 32 * sub;
            const int qa = (int)quad_unit[qbase];  // unit holding the quad's first bit (k_scan_out)
            // last slice starting at or before W0
            int lo = 0, hi = ns - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (slice_info[kSliceInfo * mid + 1] * 8 <= W0) lo = mid; else hi = mid - 1;
            }
            for (int s = lo; s < ns; ++s) {
                const uint32_t sbit = slice_info[kSliceInfo * s + 1] * 8;
                if (sbit >= W0 + 32) break;
                const uint32_t hbits = slice_info[kSliceInfo * s + 0];
                const uint32_t dend = slice_info[kSliceInfo * s + 4];
                if (sbit + slice_info[kSliceInfo * s + 2] * 8 <= W0) continue;  // slice ends before the word
                const uint32_t trail = idr ? 0u : slice_info[kSliceInfo * s + 3];
                if (sbit + hbits > W0) {
                    uint32_t hw[4] = {0, 0, 0, 0};
                    BitWriter bw;
                    bw.init(hw);
                    write_slice_header(bw, slice_params(fs, s, g.mb_w));
                    bw.flush();
                    overlap(acc, W0, sbit, hbits, [&](uint32_t x, int n) { return slot_get(hw, x, n); });
                }
                if (dend > W0 && sbit + hbits < W0 + 32) {
                    // last coded unit of the slice starting at or before W0: from the quad's
                    // first unit, forward over the (at most a few) units inside the quad
                    int a = max((int)slice_info[kSliceInfo * s + 6], qa);
                    const int rend = (int)slice_info[kSliceInfo * s + 7];
                    const int b = rend - 1;
                    while (a < b && coded_info[a + 1].x <= W0) ++a;
                    for (int r = a; r < rend; ++r) {
                        const uint4 ci = coded_info[r];
                        const uint32_t off = ci.x;
                        if (off >= W0 + 32) break;
                        if (off + ci.z <= W0) continue;
                        const int run = (int)ci.w;
                        const int plen = idr ? 0 : ue_len((uint32_t)run);
                        const uint32_t pv = (uint32_t)run + 1;
                        const uint32_t* sp = slot + (size_t)ci.y * kSlotWords;
                        overlap(acc, W0, off, ci.z, [&](uint32_t x, int n) {
                            uint32_t r2 = 0;
                            int rem = n;
                            if ((int)x < plen) {
                                const int kk = min(rem, plen - (int)x);
                                r2 = (pv >> (plen - (int)x - kk)) & mask_bits(kk);
                                rem -= kk;
                                x += kk;
                            }
                            if (rem > 0) r2 = (rem == 32 ? 0u : (r2 << rem)) | slot_get(sp, x - plen, rem);
                            return r2;
                        });
                    }
                }
                const int tl = trail ? ue_len(trail) : 0;
                const uint32_t tv = trail ? (((trail + 1) << 1) | 1u) : 1u;
                overlap(acc, W0, dend, tl + 1, [&](uint32_t x, int n) { return tv >> (tl + 1 - (int)x - n); });
            }
        }
        const uint32_t w = bswap32(acc);
        const int lane = threadIdx.x & 63, q0 = lane & ~3;
        const uint32_t w0 = __shfl(w, q0), w1 = __shfl(w, q0 + 1), w2 = __shfl(w, q0 + 2), w3 = __shfl(w, q0 + 3);
        if (active && sub == 0) out[qbase] = make_uint4(w0, w1, w2, w3);
    }
}

}  // namespace

void launch_hpel(const Geometry& g, const DeviceBuffers& b, uint8_t* const planes[4], int hp_pitch,
                 hipStream_t stream, const FrameState* publish) {
    const int W = g.coded_w + 2 * kHpelPad, H = g.coded_h + 2 * kHpelPad;
    dim3 grid((W + kHpTW - 1) / kHpTW, (H + kHpTH - 1) / kHpTH);
    const StateArg sa = make_state_arg(b, publish);
    hipLaunchKernelGGL(k_hpel, grid, dim3(256), 0, stream, g, sa, planes[0], planes[1], planes[2], planes[3],
                       hp_pitch);
}

__global__ __launch_bounds__(256) void k_copy_luma(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // 16-byte chunk
    if (i < n) dst[i] = src[i];
}

void launch_copy_luma(const Geometry& g, const uint8_t* luma, uint8_t* dst, hipStream_t stream) {
    const size_t n = (size_t)g.pitch * g.coded_h / 16;  // pitch is a multiple of 256
    hipLaunchKernelGGL(k_copy_luma, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const uint4*>(luma), reinterpret_cast<uint4*>(dst), n);
}

void launch_mc_luma_test(const Geometry& g, const uint8_t* ref, int x4, int y4, uint8_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(k_mc_luma_test, dim3(1), dim3(64), 0, stream, g, ref, x4, y4, out);
}

void launch_me(const Geometry& g, const DeviceBuffers& b, const uint8_t* src_y, hipStream_t stream,
               const FrameState* publish, bool side, const ScrollBuffers* scroll, bool quads) {
    const int nmb = g.mb_w * g.mb_h;
    const StateArg sa = make_state_arg(b, publish, !scroll);  // H.264: a P picture's first kernel, or k_scroll_probe was
    if (scroll) {
        if (side && publish)
            hipLaunchKernelGGL(quads ? k_me_full_val_scroll_q8 : k_me_full_val_scroll, dim3(nmb), dim3(kMeThreads), 0,
                               stream, g, sa, src_y, b.mb, scroll->hint);
        else
            hipLaunchKernelGGL(quads ? k_me_full_scroll_q8 : k_me_full_scroll, dim3(nmb), dim3(kMeThreads), 0, stream, g,
                               sa, src_y, b.mb, scroll->hint);
        return;
    }
    if (side && publish)
        hipLaunchKernelGGL(quads ? k_me_full_val_q8 : k_me_full_val, dim3(nmb), dim3(kMeThreads), 0, stream, g, sa,
                           src_y, b.mb);
    else
        hipLaunchKernelGGL(quads ? k_me_full_q8 : k_me_full, dim3(nmb), dim3(kMeThreads), 0, stream, g, sa, src_y, b.mb);
}

void launch_scroll_probe(const Geometry& g, const DeviceBuffers& b, const ScrollBuffers& sb, const uint8_t* src_y,
                         hipStream_t stream, const FrameState* publish) {
    const StateArg sa = make_state_arg(b, publish);
    hipLaunchKernelGGL(k_scroll_probe, dim3(scroll_probes_x(g.mb_w) * scroll_probes_y(g.mb_h)), dim3(kProbeThreads), 0,
                       stream, g, sa, src_y, sb.hist, sb.reach);
    hipLaunchKernelGGL(k_scroll_decide, dim3(1), dim3(kProbeThreads), 0, stream, sb.reach, sb.hist, sb.hint);
}

void launch_inter(const Geometry& g, const DeviceBuffers& b, const uint8_t* src_y, const uint8_t* src_uv,
                  hipStream_t stream, bool quads) {
    const int nmb = g.mb_w * g.mb_h;
    hipLaunchKernelGGL(quads ? k_inter_encode_q8 : k_inter_encode, dim3((nmb + 3) / 4), dim3(256), 0, stream, g, b.fs, src_y, src_uv, b.mb,
                       b.coef, b.mb_sse, b.wave_prog);
}

void launch_p_fused(const Geometry& g, const DeviceBuffers& b, const uint8_t* src_y, const uint8_t* src_uv,
                    hipStream_t stream, const FrameState* publish, const ScrollBuffers* scroll, bool quads) {
    const int nmb = g.mb_w * g.mb_h;
    const StateArg sa = make_state_arg(b, publish, !scroll);
    if (scroll)
        hipLaunchKernelGGL(quads ? k_p_fused_scroll_q8 : k_p_fused_scroll, dim3(nmb), dim3(kMeThreads), 0, stream, g, sa, src_y, src_uv, b.mb, b.coef,
                           b.mb_sse, b.wave_prog, scroll->hint);
    else
        hipLaunchKernelGGL(quads ? k_p_fused_q8 : k_p_fused, dim3(nmb), dim3(kMeThreads), 0, stream, g, sa, src_y, src_uv, b.mb, b.coef,
                           b.mb_sse, b.wave_prog);
}

static void launch_analyze(const Geometry& g, const DeviceBuffers& b, const uint8_t* src_y, const uint8_t* src_uv,
                           hipStream_t stream, const FrameState* publish, bool first) {
    const int nmb = g.mb_w * g.mb_h;
    // the first kernel of an I picture stamps the start; in a P picture k_me_full did
    const StateArg sa = make_state_arg(b, publish, first);
    hipLaunchKernelGGL(k_intra_analyze, dim3((nmb + 3) / 4), dim3(256), 0, stream, g, sa, src_y, src_uv, b.mb,
                       b.wave_prog, b.intra_gain, b.intra_cand);
}

void launch_intra_in_p(const Geometry& g, const DeviceBuffers& b, const uint8_t* src_y, const uint8_t* src_uv,
                       hipStream_t stream) {
    launch_analyze(g, b, src_y, src_uv, stream, nullptr, false);
    // a fixed grid over k_intra_analyze's candidate list (a few percent of the MBs)
    hipLaunchKernelGGL(k_intra_p, dim3(256), dim3(128), 0, stream, g, b.fs, src_y, src_uv, b.mb, b.coef,
                       b.intra_gain, b.mb_sse, b.wave_prog, b.intra_cand);
}

void launch_intra(const Geometry& g, const DeviceBuffers& b, const uint8_t* src_y, const uint8_t* src_uv,
                  hipStream_t stream, const FrameState* publish) {
    launch_analyze(g, b, src_y, src_uv, stream, publish, true);
    // one workgroup per (slice, plane), one wave per slice row; LDS line buffers of the rows
    const int rows = idr_slice_rows(g.mb_h), slices = (g.mb_h + rows - 1) / rows;
    const size_t lds = (size_t)rows * g.coded_w;
    // line buffers above the default dynamic-LDS limit (8K: 61 KB + tiles); per device, once
    ensure_func_attr(reinterpret_cast<const void*>(&k_intra_wave), hipFuncAttributeMaxDynamicSharedMemorySize,
                     160 * 1024 - (int)(sizeof(ChromaWaveTiles) + sizeof(LumaPipeTiles)) * 8 - 32);
    hipLaunchKernelGGL(k_intra_wave, dim3(slices, 2), dim3(64 * rows), lds, stream, g, b.fs, src_y, src_uv, b.mb,
                       b.coef);
    hipLaunchKernelGGL(k_intra_cbp, dim3((g.mb_w * g.mb_h + 255) / 256), dim3(256), 0, stream, g, b.mb);
}

__global__ __launch_bounds__(256) void k_save_src(Geometry g, const FrameState* __restrict__ fs,
                                                   const uint8_t* __restrict__ src_y) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // 16-byte chunk
    const size_t n = (size_t)g.pitch * g.coded_h / 16;
    if (i < n) reinterpret_cast<uint4*>(fs->save_src)[i] = reinterpret_cast<const uint4*>(src_y)[i];
}

void launch_save_src(const Geometry& g, const DeviceBuffers& b, const uint8_t* src_y, hipStream_t stream) {
    const size_t n = (size_t)g.pitch * g.coded_h / 16;  // pitch is a multiple of 256
    hipLaunchKernelGGL(k_save_src, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, g, b.fs, src_y);
}

void launch_entropy(const Geometry& g, const DeviceBuffers& b, uint8_t* host_out, hipStream_t stream,
                    hipEvent_t wait_for_sse, const int32_t* scroll_hint, bool quads) {
    const int nmb = g.mb_w * g.mb_h;
    hipLaunchKernelGGL(quads ? k_cavlc<true> : k_cavlc<false>, dim3((nmb + kCavlcMbPerBlock - 1) / kCavlcMbPerBlock), dim3(256), 0, stream, g, b.fs,
                       b.mb, b.coef, b.slot,
                       b.slot_bits);
    if (wait_for_sse) HIP_CHECK(hipStreamWaitEvent(stream, wait_for_sse, 0));
    if (g.mb_h > kScanMaxRows || g.mb_w > kScanThreads * kScanRowPer)
        throw std::runtime_error("launch_entropy: frame too large for the row scan");
    hipLaunchKernelGGL(quads ? k_scan_rows<true> : k_scan_rows<false>, dim3(g.mb_h), dim3(kScanThreads), 0, stream, g, b.fs, b.slot_bits, b.row_agg,
                       b.row_sse, b.mb, b.db_cnt, b.mb_sse);
    hipLaunchKernelGGL(k_scan_out, dim3(g.mb_h), dim3(kScanThreads), 0, stream, g, b.fs, b.slot_bits, b.row_agg,
                       b.row_sse, b.coded_info, b.slice_info, b.out_bytes, b.out_hdr, b.quad_unit, b.db_cnt, scroll_hint);
    hipLaunchKernelGGL(k_pack, dim3(256), dim3(256), 0, stream, g, b.fs, b.slot, b.coded_info, b.slice_info,
                       b.out_hdr, host_out, b.quad_unit, b.pack_done);
}

}  // namespace h264
}  // namespace mx
