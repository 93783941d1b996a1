// Transform-unit pipeline of the HEVC kernels (device only; gfx950, wave64): the transform
// matrices and per-wave scratch in LDS, the int16 dot products, and the stages that code_tus,
// split_tus and split4_luma (hevc_kernels.hip) compose -- forward rows, forward columns +
// quantisation, decimation, trailing trim, level store + dequantisation, inverse columns, inverse
// rows + reconstruction -- written once for every TU size.  Same integer arithmetic as
// tu_encode_t<L> of the CPU encoder (hevc_core.h), which the results must match bit for bit.
// Everything is __forceinline__ and lives in an anonymous namespace, as in common/wave.h.
//
// A TU of N x N = (1 << L)^2 coefficients occupies G = N * N / PER consecutive lanes (an aligned
// group), each lane with PER outputs per stage: idx = (lane % G) * PER + j, row idx >> L, column
// idx & (N - 1).  The stages of one TU are separated by wave_lds_sync() in the caller.
//
// Left alone on purpose: split_intra_code (one coefficient per lane, mode-dependent scan) and
// split_intra_node4 (in registers through shuffles).  Both run on the serial I-picture wavefront
// (k_hevc_intra, 256 VGPRs, occupancy 1), where latency is everything; they share level_bits only.
#pragma once

#include <hip/hip_runtime.h>

#include "../common/wave.h"
#include "hevc_core.h"

namespace mx {
namespace hevc {

namespace {

// Transform matrices in LDS (filled once per workgroup).
struct alignas(16) Mats {
    int16_t t16[256];
    int16_t t8[64];
    int16_t t4[16];
    int16_t tt16[256];  // transposed: tt16[y * 16 + k] = t16[k * 16 + y] (inverse stages)
    int16_t tt8[64];
    int16_t tt4[16];
    int16_t dst4[16];   // DST-VII of 4x4 intra luma TUs (hevc_core.h kDst4) and its transpose
    int16_t dstt4[16];
};
__device__ __forceinline__ void fill_mats(Mats& m) {
    for (int i = threadIdx.x; i < 256 + 64 + 16 + 16; i += blockDim.x) {
        if (i >= 336) {
            m.dst4[i - 336] = kDst4[i - 336];
            m.dstt4[i - 336] = kDst4[((i - 336) & 3) * 4 + ((i - 336) >> 2)];
        } else if (i < 256) {
            m.t16[i] = (int16_t)dct_coef(4, i >> 4, i & 15);
            m.tt16[i] = (int16_t)dct_coef(4, i & 15, i >> 4);
        } else if (i < 320) {
            m.t8[i - 256] = (int16_t)dct_coef(3, (i - 256) >> 3, (i - 256) & 7);
            m.tt8[i - 256] = (int16_t)dct_coef(3, (i - 256) & 7, (i - 256) >> 3);
        } else {
            m.t4[i - 320] = (int16_t)dct_coef(2, (i - 320) >> 2, (i - 320) & 3);
            m.tt4[i - 320] = (int16_t)dct_coef(2, (i - 320) & 3, (i - 320) >> 2);
        }
    }
}
// The N-point matrix of TU size L (row = frequency) and its transpose.
template <int L>
__device__ __forceinline__ const int16_t* tu_mat(const Mats& M) {
    return L == 4 ? M.t16 : (L == 3 ? M.t8 : M.t4);
}
template <int L>
__device__ __forceinline__ const int16_t* tu_mat_t(const Mats& M) {
    return L == 4 ? M.tt16 : (L == 3 ? M.tt8 : M.tt4);
}

// Integer dot products of 16 / 8 int16 pairs from 16-byte aligned LDS rows with v_dot2 (two
// multiply-adds per VALU instruction, one ds_read_b128 per 8 values).  Exact: int32 sums.
typedef short mx_short2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int dot2acc(uint32_t a, uint32_t b, int c) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(mx_short2, a), __builtin_bit_cast(mx_short2, b), c, false);
}
__device__ __forceinline__ int dot8(const int16_t* a, const int16_t* b) {
    const uint4 x = *reinterpret_cast<const uint4*>(a), y = *reinterpret_cast<const uint4*>(b);
    return dot2acc(x.w, y.w, dot2acc(x.z, y.z, dot2acc(x.y, y.y, dot2acc(x.x, y.x, 0))));
}
__device__ __forceinline__ int dot4(const int16_t* a, const int16_t* b) {  // 8-byte aligned rows
    const uint2 x = *reinterpret_cast<const uint2*>(a), y = *reinterpret_cast<const uint2*>(b);
    return dot2acc(x.y, y.y, dot2acc(x.x, y.x, 0));
}
__device__ __forceinline__ int dot16(const int16_t* a, const int16_t* b) { return dot8(a, b) + dot8(a + 8, b + 8); }
template <int N>
__device__ __forceinline__ int dotn(const int16_t* a, const int16_t* b) {
    if constexpr (N == 16) return dot16(a, b);
    if constexpr (N == 8) return dot8(a, b);
    return dot4(a, b);
}

// Per-wave TU scratch: residual / prediction / two stage buffers for 256 luma + 2 x 64 chroma
// samples.  The stages keep int16 values in a and b, laid out so that every stage reads
// contiguous rows: a = forward stage 1 transposed (aT[k][y]), then inverse stage 1 (a16[y][x]);
// b = the dequantised levels transposed (bT[x][k]).  Forward stage 1 fits 16 bits (|res| <= 255,
// row sums of |T| <= 1024 before the >> L - 1).
struct alignas(16) TuBuf {
    int16_t res[384];
    uint8_t pred[384];
    int32_t a[384];
    int32_t b[384];
};
// A TU inside its CU's TuBuf: origin and row pitch of its samples in res / pred, offset of its
// N * N stage values in a / b.
struct TuAt {
    int org, pitch, buf;
};
template <int L, int PER>
__device__ __forceinline__ int tu_idx(int j) {
    return (int)(threadIdx.x & ((1 << 2 * L) / PER - 1)) * PER + j;
}

// ---- forward stage 1 (rows): a[y][k] = sum_n T[k][n] res[y][n]
template <int L, int PER>
__device__ __forceinline__ void tu_fwd_rows(TuBuf& t, const Mats& M, TuAt u) {
    constexpr int N = 1 << L;
    int16_t* aT = reinterpret_cast<int16_t*>(t.a);
    for (int j = 0; j < PER; ++j) {
        const int idx = tu_idx<L, PER>(j), y = idx >> L, k = idx & (N - 1);
        const int s = dotn<N>(tu_mat<L>(M) + k * N, t.res + u.org + y * u.pitch);
        aT[u.buf + k * N + y] = (int16_t)((s + (1 << (L - 2))) >> (L - 1));
    }
}
// ---- forward stage 2 (columns) + quantisation: levels and their scan positions in registers
template <int L, int PER>
__device__ __forceinline__ void tu_fwd_cols_quant(const TuBuf& t, const Mats& M, TuAt u, int qp, bool intra,
                                                  int (&l)[PER], int (&si)[PER]) {
    constexpr int N = 1 << L;
    const int16_t* aT = reinterpret_cast<const int16_t*>(t.a);
    for (int j = 0; j < PER; ++j) {
        const int idx = tu_idx<L, PER>(j), k2 = idx >> L, k = idx & (N - 1);
        const int s = dotn<N>(tu_mat<L>(M) + k2 * N, aT + u.buf + k * N);
        l[j] = quant_coef((s + (1 << (L + 5))) >> (L + 6), qp, L, intra);
        si[j] = scan_index(L, k, k2);
    }
}
// Group reductions of the two rules below.  kQuad (G == 4 only): the group is the lane's DPP quad, so
// the reduction is four quad_perm moves on the VALU and stays off the LDS crossbar that the
// xor-shuffle ladder of gsum / gmax goes through -- the transform-skip candidate reduces this way
// while the transformed candidate's ds_read / v_dot2 stages own the LDS pipe.
__device__ __forceinline__ int quad_max(int v) { return max(max(qbc<0>(v), qbc<1>(v)), max(qbc<2>(v), qbc<3>(v))); }
template <int G, bool kQuad>
__device__ __forceinline__ int tu_gsum(int v) {
    if constexpr (kQuad) return quad_sum(v);
    else return gsum<G>(v);
}
template <int G, bool kQuad>
__device__ __forceinline__ int tu_gmax(int v) {
    if constexpr (kQuad) return quad_max(v);
    else return gmax<G>(v);
}
// Decimation of the TU on this lane's aligned group of G lanes (tu_decimate, group-uniform).
template <int G, int N, bool kQuad = false>
__device__ __forceinline__ void tu_decimate_group(int (&l)[N], int log2n, bool intra) {
    static_assert(!kQuad || G == 4, "a quad is four lanes");
    int nz = 0, mx = 0;
    for (int j = 0; j < N; ++j) {
        nz += l[j] != 0;
        mx = max(mx, abs(l[j]));
    }
    if (tu_decimate(log2n, intra, tu_gsum<G, kQuad>(nz), tu_gmax<G, kQuad>(mx)))
        for (int j = 0; j < N; ++j) l[j] = 0;
}
// Trailing isolated +-1 trim of the TU on this lane's group (tu_encode_t rule): the lane owning
// the last level clears it; a stopped TU stays stopped, and the loop ends once every TU of the
// wave has stopped.  Called by the whole wave.
template <int G, int N, bool kQuad = false>
__device__ __forceinline__ void tu_trim_group(int (&l)[N], const int (&si)[N]) {
    bool on = true;
    for (int it = 0; it < kTrimIters; ++it) {
        int last = -1;
        for (int j = 0; j < N; ++j)
            if (l[j]) last = max(last, si[j]);
        last = tu_gmax<G, kQuad>(last);
        int prev = -1, lv = 0;
        for (int j = 0; j < N; ++j) {
            if (l[j] && si[j] < last) prev = max(prev, si[j]);
            if (l[j] && si[j] == last) lv = abs(l[j]);
        }
        prev = tu_gmax<G, kQuad>(prev);
        lv = tu_gmax<G, kQuad>(lv);
        if (last < 0 || lv != 1 || last - prev <= kTrimGap) on = false;
        if (!__any(on)) break;
        if (on)
            for (int j = 0; j < N; ++j)
                if (si[j] == last) l[j] = 0;
    }
}
// ---- levels to lv (the TU's levels in scan order), dequantised values to b; the lane's count
// of coded levels and their level_bits are added to nz / bits
template <int L, int PER>
__device__ __forceinline__ void tu_store_dequant(TuBuf& t, TuAt u, int qp, const int (&l)[PER], const int (&si)[PER],
                                                 int16_t* lv, int& nz, int& bits) {
    constexpr int N = 1 << L;
    int16_t* bT = reinterpret_cast<int16_t*>(t.b);
    for (int j = 0; j < PER; ++j) {
        const int idx = tu_idx<L, PER>(j), k2 = idx >> L, k = idx & (N - 1);
        lv[si[j]] = (int16_t)l[j];
        bT[u.buf + k * N + k2] = (int16_t)dequant_coef(l[j], qp, L);
        nz += l[j] != 0;
        bits += level_bits(l[j]);
    }
}
// ---- inverse stage 1 (columns): a[y][x] = clip16((sum_k T[k][y] b[k][x] + 64) >> 7)
template <int L, int PER>
__device__ __forceinline__ void tu_inv_cols(TuBuf& t, const Mats& M, TuAt u) {
    constexpr int N = 1 << L;
    int16_t* a16 = reinterpret_cast<int16_t*>(t.a);
    const int16_t* bT = reinterpret_cast<const int16_t*>(t.b);
    for (int j = 0; j < PER; ++j) {
        const int idx = tu_idx<L, PER>(j), y = idx >> L, x = idx & (N - 1);
        const int s = dotn<N>(tu_mat_t<L>(M) + y * N, bT + u.buf + x * N);
        a16[u.buf + idx] = (int16_t)clip16((s + 64) >> 7);
    }
}
// ---- inverse stage 2 (rows) + reconstruction (a TU without levels keeps its prediction).  Every
// sample goes to emit(y, x, o, v, e2): position inside the TU, offset in res / pred,
// reconstructed value and squared error against the source.
template <int L, int PER, class Emit>
__device__ __forceinline__ void tu_inv_rows_rec(const TuBuf& t, const Mats& M, TuAt u, bool coded, Emit emit) {
    constexpr int N = 1 << L;
    const int16_t* a16 = reinterpret_cast<const int16_t*>(t.a);
    for (int j = 0; j < PER; ++j) {
        const int idx = tu_idx<L, PER>(j), y = idx >> L, x = idx & (N - 1);
        const int s = dotn<N>(tu_mat_t<L>(M) + x * N, a16 + u.buf + y * N);
        const int r = coded ? (s + 2048) >> 12 : 0;
        const int o = u.org + y * u.pitch + x, p = t.pred[o];
        const int v = clip255(p + r), e = p + t.res[o] - v;
        emit(y, x, o, v, e * e);
    }
}

// ---- the transform-skip candidate of a 4x4 luma TU (tu4_skip_encode of hevc_core.h), on the lanes
// of the <2, 4> stages: four lanes per TU, lane q of the quad owns row q -- coefficients (q, 0..3) in
// the transformed candidate, samples (q, 0..3) here, so both candidates' levels sit at the same scan
// positions si[] of the same lane.  The candidate has no matrix and no stage buffer: one 8-byte read
// of the lane's residual row, one 4-byte read of its prediction row, everything else in registers
// and quad DPP.  Its steps carry no LDS dependence on the transformed candidate's stages, so the
// caller places them between those stages' wave_lds_sync() phases, where they fill the ds_read_b128 /
// v_dot2 latency.
struct Skip4 {
    int l[4];       // levels of samples (q, 0..3)
    uint32_t rec;   // the row's reconstructed samples, one byte each
    int sse, disp;  // squared error of the row: whole / inside the display area
    int nz, bits;   // the TU's coded levels and their level_bits (quad-uniform)
};
__device__ __forceinline__ uint2 tu4_row_res(const TuBuf& t, TuAt u) {
    return *reinterpret_cast<const uint2*>(t.res + u.org + (int)(threadIdx.x & 3) * u.pitch);
}
__device__ __forceinline__ int tu4_row_sample(uint2 w, int j) {
    return (int)(int16_t)(((j & 2) ? w.y : w.x) >> ((j & 1) * 16));
}
// forward "transform" + quantisation
__device__ __forceinline__ void tu4_skip_quant(const TuBuf& t, TuAt u, int qp, Skip4& s) {
    const uint2 w = tu4_row_res(t, u);
#pragma unroll
    for (int j = 0; j < 4; ++j) s.l[j] = quant_coef(tskip_fwd(tu4_row_sample(w, j)), qp, 2, false);
}
// decimation and trailing trim on the quad; si: the lane's scan positions (tu_fwd_cols_quant<2, 4>)
__device__ __forceinline__ void tu4_skip_trim(Skip4& s, const int (&si)[4]) {
    tu_decimate_group<4, 4, true>(s.l, 2, false);
    tu_trim_group<4, 4, true>(s.l, si);
    int nz = 0, b = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        nz += s.l[j] != 0;
        b += level_bits(s.l[j]);
    }
    s.nz = quad_sum(nz);
    s.bits = quad_sum(b);
}
// dequantisation + reconstruction of the lane's row; in_disp(x): column x of the TU is displayed
template <class InDisp>
__device__ __forceinline__ void tu4_skip_rec(const TuBuf& t, TuAt u, int qp, Skip4& s, InDisp in_disp) {
    const uint2 w = tu4_row_res(t, u);
    const uint32_t pw = *reinterpret_cast<const uint32_t*>(t.pred + u.org + (int)(threadIdx.x & 3) * u.pitch);
    s.rec = 0;
    s.sse = s.disp = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = (int)((pw >> (8 * j)) & 0xffu);
        const int v = clip255(p + tskip_inv(dequant_coef(s.l[j], qp, 2)));
        const int e = p + tu4_row_sample(w, j) - v;
        s.rec |= (uint32_t)v << (8 * j);
        s.sse += e * e;
        s.disp += in_disp(j) ? e * e : 0;
    }
}

}  // namespace

}  // namespace hevc
}  // namespace mx
