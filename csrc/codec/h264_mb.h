// Macroblock-level syntax helpers shared by the HIP kernels and the CPU encoder:
// neighbour availability, nC prediction, motion-vector prediction / P_Skip decision and
// the per-"role" CAVLC coding of one macroblock (role 0 = header, 1 = Intra16x16 DC,
// 2..17 = luma 4x4 blocks in blkIdx order, 18/19 = chroma DC, 20..27 = chroma AC).
// Coding roles in ascending order reproduces macroblock_layer() syntax order.
#pragma once
#include "h264_core.h"
#include "h264_gpu.h"
#include "h264_intra.h"

namespace mx {
namespace h264 {

constexpr int kNumRoles = 28;

struct Avail {
    bool left, top, topright, topleft;
};

MXHD Avail mb_avail(const Geometry& g, int mbx, int mby, int slice_rows) {
    Avail a;
    const bool top_same_slice = mby > 0 && (mby / slice_rows) == ((mby - 1) / slice_rows);
    a.left = mbx > 0;
    a.top = top_same_slice;
    a.topright = top_same_slice && mbx < g.mb_w - 1;
    a.topleft = top_same_slice && mbx > 0;
    return a;
}

MXHD int combine_nc(bool ha, int na, bool hb, int nb) {
    if (ha && hb) return (na + nb + 1) >> 1;
    if (ha) return na;
    if (hb) return nb;
    return 0;
}

// A macroblock and its neighbours (left, top, top-right, top-left) as the entropy coder reads
// them: pointers into the frame's MbInfo array (CPU) or into LDS copies (k_cavlc).  A pointer
// is only dereferenced when the neighbour is available.
struct MbNbrs {
    const MbInfo* self;
    const MbInfo* left;
    const MbInfo* top;
    const MbInfo* topright;
    const MbInfo* topleft;
};
MXHD MbNbrs mb_nbrs(const MbInfo* mbs, int mbi, int mb_w) {
    return MbNbrs{&mbs[mbi], &mbs[mbi - 1], &mbs[mbi - mb_w], &mbs[mbi - mb_w + 1], &mbs[mbi - mb_w - 1]};
}

// Vector of 4x4 block (bx, by) of an inter macroblock (partition-aware).  kQuad false: the caller
// knows that the macroblock is not P_8x8 (a coder kernel of a picture searched without quadrants).
template <bool kQuad = true>
MXHD Mv blk_mv(const MbInfo& m, int bx, int by) {
    if (m.part == kPart16x8) return by < 2 ? Mv{m.pmv[0], m.pmv[1]} : Mv{m.pmv[2], m.pmv[3]};
    if (m.part == kPart8x16) return bx < 2 ? Mv{m.pmv[0], m.pmv[1]} : Mv{m.pmv[2], m.pmv[3]};
    if (kQuad && m.part == kPart8x8) {  // quadrant 0 TL, 1 TR, 2 BL, 3 BR (the layout: h264_gpu.h MbInfo)
        // the four vectors read first, then chosen by value (a choice between the fields' addresses
        // would keep the whole MbInfo in scratch memory on the GPU)
        const int x0 = m.mvx, y0 = m.mvy, x1 = m.pmv[0], y1 = m.pmv[1], x2 = m.pmv[2], y2 = m.pmv[3], x3 = m.pmv3[0], y3 = m.pmv3[1];
        const bool right = bx >= 2, low = by >= 2;
        return Mv{low ? (right ? x3 : x2) : (right ? x1 : x0), low ? (right ? y3 : y2) : (right ? y1 : y0)};
    }
    return Mv{m.mvx, m.mvy};
}
// Vector of quadrant q of a P_8x8 macroblock, and storing it.
MXHD Mv quad_mv(const MbInfo& m, int q) { return blk_mv(m, 2 * (q & 1), q & 2); }
MXHD void set_quad_mv(MbInfo& m, int q, int vx, int vy) {
    if (q == 0) {
        m.mvx = (int16_t)vx;
        m.mvy = (int16_t)vy;
    } else {
        int16_t* p = q == 3 ? m.pmv3 : m.pmv + 2 * (q - 1);
        p[0] = (int16_t)vx;
        p[1] = (int16_t)vy;
    }
}
// Vector of luma sample (x, y) of the macroblock.
template <bool kQuad = true>
MXHD Mv px_mv(const MbInfo& m, int x, int y) { return blk_mv<kQuad>(m, x >> 2, y >> 2); }

// Neighbour for motion-vector prediction: block (bx, by) of macroblock p.  (kQuad through the
// functions below: as blk_mv -- false where no macroblock of the picture is P_8x8, k_cavlc.)
template <bool kQuad = true>
MXHD MvNb mv_nb_blk(const MbInfo* p, bool avail, int bx, int by) {
    MvNb n;
    n.avail = avail;
    n.ref = -1;
    n.mv = Mv{0, 0};
    if (!avail) return n;
    const MbInfo& m = *p;
    if (m.type == kMbP16x16) {
        n.ref = 0;
        n.mv = blk_mv<kQuad>(m, bx, by);
    }
    return n;
}

// 8.4.1.3 prediction of partition `idx` (0 / 1) of a 16x8 / 8x16 macroblock: neighbours A, B, C
// of the partition (C replaced by D when unavailable; blocks of the right neighbour are never
// available yet), the directional rules, else the median.  mv0: this MB's partition 0 vector.
template <bool kQuad = true>
MXHD Mv predict_mv_part(const MbNbrs& nb, const Avail& av, int part, int idx, Mv mv0) {
    MvNb own;
    own.avail = true;
    own.ref = 0;
    own.mv = mv0;
    MvNb a, b, c;
    if (part == kPart16x8) {
        if (idx == 0) {
            a = mv_nb_blk<kQuad>(nb.left, av.left, 3, 0);
            b = mv_nb_blk<kQuad>(nb.top, av.top, 0, 3);
            c = av.topright ? mv_nb_blk<kQuad>(nb.topright, true, 0, 3) : mv_nb_blk<kQuad>(nb.topleft, av.topleft, 3, 3);
            if (b.ref == 0) return b.mv;
        } else {
            a = mv_nb_blk<kQuad>(nb.left, av.left, 3, 2);
            b = own;
            c = mv_nb_blk<kQuad>(nb.left, av.left, 3, 1);  // C = (16, 7) not yet decoded -> D = (-1, 7)
            if (a.ref == 0) return a.mv;
        }
    } else {
        if (idx == 0) {
            a = mv_nb_blk<kQuad>(nb.left, av.left, 3, 0);
            b = mv_nb_blk<kQuad>(nb.top, av.top, 0, 3);
            c = av.top ? mv_nb_blk<kQuad>(nb.top, true, 2, 3) : mv_nb_blk<kQuad>(nb.topleft, av.topleft, 3, 3);
            if (a.ref == 0) return a.mv;
        } else {
            a = own;
            b = mv_nb_blk<kQuad>(nb.top, av.top, 2, 3);
            c = av.topright ? mv_nb_blk<kQuad>(nb.topright, true, 0, 3) : mv_nb_blk<kQuad>(nb.top, av.top, 1, 3);
            if (c.ref == 0) return c.mv;
        }
    }
    return predict_mv16x16(a, b, c);
}

// 8.4.1.3 prediction of quadrant q (0 TL, 1 TR, 2 BL, 3 BR) of a P_8x8 macroblock: the plain median
// of neighbours A, B, C (C replaced by D when unavailable), no directional rule.  The quadrants
// before q are this macroblock's own (read through blk_mv: they are final when q is predicted).
//   q | A              | B              | C, and D when C is unavailable
//   0 | left MB (3, 0) | top MB (0, 3)  | top MB (2, 3); top-left MB (3, 3) when the top is unavailable
//   1 | quadrant 0     | top MB (2, 3)  | top-right MB (0, 3); else top MB (1, 3)
//   2 | left MB (3, 2) | quadrant 0     | quadrant 1
//   3 | quadrant 2     | quadrant 1     | not yet decoded -> quadrant 0
MXHD Mv predict_mv_quad(const MbNbrs& nb, const Avail& av, int q) {
    auto own = [&](int k) {
        MvNb n;
        n.avail = true;
        n.ref = 0;
        n.mv = quad_mv(*nb.self, k);
        return n;
    };
    MvNb a, b, c;
    if (q == 0) {
        a = mv_nb_blk(nb.left, av.left, 3, 0);
        b = mv_nb_blk(nb.top, av.top, 0, 3);
        c = av.top ? mv_nb_blk(nb.top, true, 2, 3) : mv_nb_blk(nb.topleft, av.topleft, 3, 3);
    } else if (q == 1) {
        a = own(0);
        b = mv_nb_blk(nb.top, av.top, 2, 3);
        c = av.topright ? mv_nb_blk(nb.topright, true, 0, 3) : mv_nb_blk(nb.top, av.top, 1, 3);
    } else if (q == 2) {
        a = mv_nb_blk(nb.left, av.left, 3, 2);
        b = own(0);
        c = own(1);
    } else {
        a = own(2);
        b = own(1);
        c = own(0);
    }
    return predict_mv16x16(a, b, c);
}

// P_Skip decision + the motion vector differences of a P macroblock: mvd[0..1] (16x16, partition 0
// or quadrant 0), mvd[2..3] (partition 1 or quadrant 1), mvd[4..7] (quadrants 2, 3).  Returns true
// for P_Skip (16x16 only).
// kQuad false: mvd has four entries.
template <bool kQuad = true>
MXHD bool decide_skip(const MbNbrs& nb, const Avail& av, int* mvd) {
    const MbInfo& m = *nb.self;
    mvd[0] = mvd[1] = mvd[2] = mvd[3] = 0;
    if (kQuad) mvd[4] = mvd[5] = mvd[6] = mvd[7] = 0;
    if (m.type != kMbP16x16) return false;
    if (kQuad && m.part == kPart8x8) {
        for (int q = 0; q < 4; ++q) {
            const Mv v = quad_mv(m, q), p = predict_mv_quad(nb, av, q);
            mvd[2 * q] = v.x - p.x;
            mvd[2 * q + 1] = v.y - p.y;
        }
        return false;
    }
    if (m.part != kPart16x16) {
        const Mv v0{m.pmv[0], m.pmv[1]}, v1{m.pmv[2], m.pmv[3]};
        const Mv p0 = predict_mv_part<kQuad>(nb, av, m.part, 0, v0);
        const Mv p1 = predict_mv_part<kQuad>(nb, av, m.part, 1, v0);
        mvd[0] = v0.x - p0.x;
        mvd[1] = v0.y - p0.y;
        mvd[2] = v1.x - p1.x;
        mvd[3] = v1.y - p1.y;
        return false;
    }
    const MvNb a = mv_nb_blk<kQuad>(nb.left, av.left, 3, 0);
    const MvNb b = mv_nb_blk<kQuad>(nb.top, av.top, 0, 3);
    MvNb c = mv_nb_blk<kQuad>(nb.topright, av.topright, 0, 3);
    if (!av.topright) c = mv_nb_blk<kQuad>(nb.topleft, av.topleft, 3, 3);
    const Mv pskip = predict_mv_skip(a, b, c);
    const Mv p = predict_mv16x16(a, b, c);
    mvd[0] = m.mvx - p.x;
    mvd[1] = m.mvy - p.y;
    return m.cbp == 0 && m.mvx == pskip.x && m.mvy == pskip.y;
}

template <bool kQuad = true, class W>
MXHD void code_role(W& w, int role, const Geometry& g, int idr, const MbNbrs& nb, const int16_t* mc,
                    const Avail& av, const int* mvd, int dqp = 0) {
    const MbInfo& m = *nb.self;
    const bool intra = m.type == kMbI16x16;  // Intra16x16: DC / AC split of the luma residual
    const int cbp = m.cbp;
    const int cbp_l = cbp & 15, cbp_c = cbp >> 4;
    const MbInfo* ml = av.left ? nb.left : nullptr;
    const MbInfo* mt = av.top ? nb.top : nullptr;
    if (role == 0) {
        if (intra) {
            const int mbtype = 1 + m.i16_mode + 4 * cbp_c + (cbp_l ? 12 : 0);
            put_ue(w, (uint32_t)(idr ? mbtype : 5 + mbtype));
            put_ue(w, m.chroma_mode);
            put_se(w, dqp);  // mb_qp_delta (0 in I slices: every MB at the slice QP)
        } else if (m.type == kMbI4x4) {
            put_ue(w, idr ? 0u : 5u);  // I_NxN
            // prev_intra4x4_pred_mode_flag / rem_intra4x4_pred_mode, blkIdx order (8.3.1.1:
            // a neighbour MB that is not Intra4x4 counts as DC, an unavailable one forces DC)
            for (int b = 0; b < 16; ++b) {
                const int bx = kBlkX[b], by = kBlkY[b];
                const bool ha = bx > 0 || av.left, hb = by > 0 || av.top;
                int ma = -1, mb = -1;
                if (bx > 0) ma = i4_get(m.i4, by * 4 + bx - 1);
                else if (ml && ml->type == kMbI4x4) ma = i4_get(ml->i4, by * 4 + 3);
                if (by > 0) mb = i4_get(m.i4, (by - 1) * 4 + bx);
                else if (mt && mt->type == kMbI4x4) mb = i4_get(mt->i4, 12 + bx);
                const int pm = i4_pred_mode(ma, mb, ha, hb);
                const int mode = i4_get(m.i4, by * 4 + bx);
                if (mode == pm) {
                    w.put(1, 1);
                } else {
                    w.put(0, 1);
                    w.put((uint32_t)(mode < pm ? mode : mode - 1), 3);
                }
            }
            put_ue(w, m.chroma_mode);
            put_ue(w, (uint32_t)cbp_to_codenum(cbp, true));
            if (cbp) put_se(w, dqp);
        } else {
            put_ue(w, m.part);  // P_L0_16x16 / P_L0_L0_16x8 / P_L0_L0_8x16 / P_8x8 (one reference: no ref_idx)
            if (kQuad && m.part == kPart8x8)
                for (int q = 0; q < 4; ++q) put_ue(w, 0u);  // sub_mb_type P_L0_8x8
            put_se(w, mvd[0]);
            put_se(w, mvd[1]);
            if (m.part != kPart16x16) {
                put_se(w, mvd[2]);
                put_se(w, mvd[3]);
            }
            if (kQuad && m.part == kPart8x8)
                for (int i = 4; i < 8; ++i) put_se(w, mvd[i]);
            put_ue(w, (uint32_t)cbp_to_codenum(cbp, false));
            if (cbp) put_se(w, dqp);  // mb_qp_delta (adaptive quantisation)
        }
        return;
    }
    if (role == 1) {
        if (!intra) return;
        const int nc = combine_nc(av.left, ml ? ml->nz_luma[3] : 0, av.top, mt ? mt->nz_luma[12] : 0);
        cavlc_block(w, mc + kCoefLumaDc, 16, nc);
        return;
    }
    if (role <= 17) {
        const int b = role - 2;
        if (!(cbp_l & (1 << (b >> 2)))) return;
        const int bx = kBlkX[b], by = kBlkY[b];
        const bool ha = bx > 0 || av.left, hb = by > 0 || av.top;
        const int na = bx > 0 ? m.nz_luma[by * 4 + bx - 1] : (ml ? ml->nz_luma[by * 4 + 3] : 0);
        const int nb = by > 0 ? m.nz_luma[(by - 1) * 4 + bx] : (mt ? mt->nz_luma[12 + bx] : 0);
        const int nc = combine_nc(ha, na, hb, nb);
        if (intra) {
            cavlc_block(w, mc + kCoefLuma + b * 16 + 1, 15, nc);  // AC only (DC in the Intra16x16 DC block)
        } else {
            cavlc_block(w, mc + kCoefLuma + b * 16, 16, nc);
        }
        return;
    }
    if (role <= 19) {
        if (!cbp_c) return;
        const int comp = role - 18;
        cavlc_block(w, mc + kCoefChromaDc + comp * 4, 4, -1);
        return;
    }
    if (role < kNumRoles) {
        if (cbp_c != 2) return;
        const int comp = (role - 20) >> 2, cb = (role - 20) & 3, bx = cb & 1, by = cb >> 1;
        const uint8_t* own = comp ? m.nz_cr : m.nz_cb;
        const uint8_t* lft = ml ? (comp ? ml->nz_cr : ml->nz_cb) : nullptr;
        const uint8_t* top = mt ? (comp ? mt->nz_cr : mt->nz_cb) : nullptr;
        const bool ha = bx > 0 || av.left, hb = by > 0 || av.top;
        const int na = bx > 0 ? own[by * 2] : (lft ? lft[by * 2 + 1] : 0);
        const int nb = by > 0 ? own[bx] : (top ? top[2 + bx] : 0);
        const int nc = combine_nc(ha, na, hb, nb);
        cavlc_block(w, mc + kCoefChromaAc + (comp * 4 + cb) * 16 + 1, 15, nc);
    }
}

// Adaptive quantisation (residual-energy based, P macroblocks): a block whose motion-
// compensated luma residual stays noise-like (mean |residual| above 32 / 48 per pixel) is
// quantised 6 / 12 QP coarser -- refining incompressible content costs far more bits than
// it returns -- and the rate controller hands those bits to the rest of the picture (text,
// UI edges).  sad = sum |src - pred| over the 16x16 luma block.
MXHD int aq_mb_qp(int frame_qp, uint32_t sad, int aq) {
    if (!aq) return frame_qp;  // (aq 3 -- the temporal classes below -- falls back to this rule in HEVC)
    const int off = sad > 256u * 48 ? 12 : (sad > 256u * 32 ? 6 : 0);
    const int q = frame_qp + off;
    return q > 51 ? 51 : q;
}

// Rate-distortion residual drop for noise-like P macroblocks (EncoderConfig::aq >= 2).  A
// macroblock in an AQ noise class (mean |luma residual| above 32 per pixel) keeps its residual
// only if coding it lowers the luma distortion by more than lambda * (estimated bits):
// refining incompressible content at the QPs a CBR budget allows costs far more than it
// returns, and the rate controller hands those bits to the rest of the picture.  lambda is
// the H.264 reference mode-decision lambda 0.85 * 2^((qp - 12) / 3) (SSE domain), the bit
// estimate 2 + 6 per non-zero coefficient per 4x4 block.
MXHD int lambda_sse(int qp) {
    constexpr int tab[52] = {0,   0,   0,   0,   0,   0,   0,   0,   0,    0,    1,    1,    1,    1,
                             1,   2,   2,   3,   3,   4,   5,   7,   9,    11,   14,   17,   22,   27,
                             34,  43,  54,  69,  86,  109, 137, 173, 218,  274,  345,  435,  548,  691,
                             870, 1097, 1382, 1741, 2193, 2763, 3482, 4387, 5527, 6963};
    return tab[qp < 0 ? 0 : (qp > 51 ? 51 : qp)];
}
MXHD uint32_t block_bits_est(int nz) { return nz ? 2u + 6u * (uint32_t)nz : 0u; }
MXHD bool drop_residual(int aq, uint32_t lsad, int qp, long long d_pred, long long d_coded, uint32_t bits) {
    if (aq < 2 || lsad <= 256u * 32) return false;
    return d_pred - d_coded < (long long)lambda_sse(qp) * (long long)bits;
}

// Temporal classes (EncoderConfig::aq == 3, the H.264 default).  The residual-energy rule above
// cannot tell incompressible content from well-predictable content whose reference is still
// coarse: text coded at a high QP in the IDR leaves a large residual too, and was then quantised
// 6-12 QP coarser -- never refined (the document window stayed at 28 dB over the driver window,
// tools/region_report.py).  The classes here use the SOURCE's own temporal change instead:
// tsad = sum |src_n - src_(n-1)| over the 16x16 luma block displaced by the integer part of the
// chosen motion vector.
//  * changing content (tsad > 24 / pixel: e.g. animated noise, video): its bits are thrown away
//    with the next picture -> 6 QP coarser, luma residual kept only if it pays for its bits
//    (drop_residual's rate-distortion rule), chroma residual dropped;
//  * persistent content (tsad <= 2 / pixel: static or moving rigidly): everything coded now is
//    re-used by every later picture (the static desktop refines once and is then skipped) ->
//    6 QP finer -- a one-step form of x264's macroblock-tree propagation without a lookahead;
//  * anything else at the frame QP.
constexpr uint32_t kTsadChanging = 256u * 24, kTsadPersistent = 256u * 2;
constexpr int kAqChangingOffset = 6, kAqPersistentOffset = -6;
// Static content (aq >= 4): a block whose source is bit-identical to the previous source with a zero
// vector is coded once and then skipped for as long as it stays -- refined 9 / 12 / 15 QP finer
// (aq 4 / 5 / 6) than the frame QP; only rigidly MOVING persistent content (a pan, a scroll) keeps
// -6, since there every frame re-spends the finer QP on the newly exposed / re-predicted blocks and
// the rate control raises the frame QP for everything (profiles/r04_hevc/NOTES.md: aq 5 on the
// motion content cost 5 dB when the offset applied to every persistent block).
MXHD int aq_static_offset(int aq) { return kAqPersistentOffset - 3 * ((aq > 6 ? 6 : aq) - 3); }
enum TClass : int { kTcNormal = 0, kTcPersistent = 1, kTcChanging = 2, kTcStatic = 3 };
MXHD int temporal_class(uint32_t tsad, bool zero_mv) {
    return tsad > kTsadChanging ? kTcChanging
                                : (tsad == 0 && zero_mv ? kTcStatic : (tsad <= kTsadPersistent ? kTcPersistent : kTcNormal));
}
MXHD int aq3_mb_qp(int frame_qp, int tclass, int aq = 3) {
    const int q = frame_qp + (tclass == kTcChanging     ? kAqChangingOffset
                              : tclass == kTcStatic     ? aq_static_offset(aq)
                              : tclass == kTcPersistent ? kAqPersistentOffset
                                                        : 0);
    return q < 0 ? 0 : (q > 51 ? 51 : q);
}
// MB QP and residual-drop decision of a P macroblock for any aq mode (aq >= 3 uses tclass).
MXHD int mb_qp_for(int frame_qp, uint32_t lsad, int tclass, int aq) {
    return aq >= 3 ? aq3_mb_qp(frame_qp, tclass, aq) : aq_mb_qp(frame_qp, lsad, aq);
}
MXHD bool drop_luma_for(int aq, uint32_t lsad, int tclass, int qp, long long d_pred, long long d_coded,
                        uint32_t bits) {
    if (aq >= 3)
        return tclass == kTcChanging && d_pred - d_coded < (long long)lambda_sse(qp) * (long long)bits;
    return drop_residual(aq, lsad, qp, d_pred, d_coded, bits);
}
// Whether drop_luma_for can return true at all for this macroblock: only then are its distortion
// and bit-estimate arguments needed.
MXHD bool drop_luma_possible(int aq, uint32_t lsad, int tclass) {
    return aq >= 3 ? tclass == kTcChanging : (aq >= 2 && lsad > 256u * 32);
}
MXHD bool drop_chroma_for(int aq, int tclass, bool luma_dropped) {
    return luma_dropped || (aq >= 3 && tclass == kTcChanging);
}

// Inter cost of a P16x16 macroblock for the intra decision: luma SATD of the motion-
// compensated residual + mv rate at the frame lambda.
MXHD uint32_t inter_cost(uint32_t satd, int frame_qp, int mvx, int mvy) {
    return satd + (uint32_t)(lambda_sad(frame_qp) * (mvd_bits(mvx) + mvd_bits(mvy)));
}
// ... of a partitioned macroblock: both vectors' rate, or all four (kQuad: as blk_mv)
template <bool kQuad = true>
MXHD uint32_t inter_cost_mb(uint32_t satd, int frame_qp, const MbInfo& m) {
    if (m.part == kPart16x16) return inter_cost(satd, frame_qp, m.mvx, m.mvy);
    if (kQuad && m.part == kPart8x8) {  // all eight components
        int bits = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const Mv v = quad_mv(m, q);
            bits += mvd_bits(v.x) + mvd_bits(v.y);
        }
        return satd + (uint32_t)(lambda_sad(frame_qp) * bits);
    }
    return satd + (uint32_t)(lambda_sad(frame_qp) *
                             (mvd_bits(m.pmv[0]) + mvd_bits(m.pmv[1]) + mvd_bits(m.pmv[2]) + mvd_bits(m.pmv[3])));
}

// Rows per slice of an IDR picture: intra macroblocks are reconstructed in a diagonal
// wavefront per slice (one workgroup per slice, one wave per row, k_intra_wave), so a slice
// takes about as long as its most expensive MB row plus a 2-MB lag per row.  <= 4-row slices
// (17 at 1080p) keep one row wave per SIMD and spread the text-heavy rows over more
// workgroups: 1,059 -> 914 us per 1080p IDR against 8-row slices for +0.7 % IDR bytes
// (profiles/r02_idr).
MXHD int idr_slice_rows(int mb_h) {
    const int ns = (mb_h + 3) / 4;  // <= 4 rows
    return (mb_h + ns - 1) / ns;
}

// mb_qp_delta value for QP `qp` after predictor `pred` (both 0..51), in -26..25.
MXHD int qp_delta(int qp, int pred) { return ((qp - pred + 26 + 52) % 52) - 26; }

MXHD SliceParams make_slice_params(int first_mb, int idr, int frame_num, int log2_max_frame_num, int idr_pic_id,
                                   int qp_delta, int deblock_off) {
    SliceParams sp;
    sp.first_mb = first_mb;
    sp.idr = idr;
    sp.frame_num = frame_num;
    sp.log2_max_frame_num = log2_max_frame_num;
    sp.idr_pic_id = idr_pic_id;
    sp.qp_delta = qp_delta;
    sp.disable_deblock = deblock_off;
    return sp;
}

// ---- per-block transform pipelines (same arithmetic on both encoders)

// Inter luma block: residual (raster) -> levels (scan order) + reconstructed residual.
MXHD int luma_block_inter(const int* res, int qp, int* zscan, int* rres) {
    int y[16], z[16], d[16];
    fdct4x4(res, y);
    const int nz = quant4x4(y, z, qp, false, 0);
    for (int k = 0; k < 16; ++k) zscan[k] = z[kZigzag4x4[k]];
    dequant4x4(z, d, qp, 0);
    idct4x4(d, rres);
    return nz;
}

// ---- residuals that are known to quantise to all-zero levels without running a transform
// A coefficient of fdct4x4 is a sum of the block's 16 residuals with weights a(i) * a(j), a = 1 on
// the even and 2 on the odd basis rows ({1,1,1,1}, {2,1,-1,-2}, {1,-1,-1,1}, {1,-2,2,-1}), so with
// S = sum |residual| over the block, |coefficient (i, j)| <= a(i) a(j) S.  quant4x4 (inter dead
// zone f) gives level 0 while |c| * MF + f < 2^qbits, hence every level of the block is 0 when
// S <= min over the 16 positions of (2^qbits - 1 - f) / (a(i) a(j) MF[qp % 6][class]).  The
// chroma DC coefficients of a plane are +-sums of its four blocks' DC terms (weight 1 each), so
// they are bounded by the plane's sum over its 8x8 samples, against quant_dc_chroma's f and qbits.
// A bound of 0 (low QPs) leaves only the all-zero block.  Sufficient, not necessary.
constexpr int fdct_row_gain(int i) { return (i & 1) ? 2 : 1; }
constexpr int zero_sum_4x4_calc(int qp) {
    const int qm = qp % 6, qbits = 15 + qp / 6;
    const int room = (1 << qbits) - 1 - (1 << qbits) / 6;  // quant4x4, inter
    int t = room;
    for (int i = 0; i < 16; ++i) {
        const int b = room / (fdct_row_gain(i >> 2) * fdct_row_gain(i & 3) * kQuantMF[qm][kPosClass[i]]);
        t = b < t ? b : t;
    }
    return t;
}
constexpr int zero_sum_chroma_dc_calc(int qpc) {
    const int qm = qpc % 6, qbits = 16 + qpc / 6;
    const int room = (1 << qbits) - 1 - 2 * ((1 << (qbits - 1)) / 6);  // quant_dc_chroma, inter
    return room / kQuantMF[qm][0];
}
struct ZeroSumTab {
    uint16_t blk[52], cdc[52];  // blk <= 16 * 255 matters, cdc <= 64 * 255: saturated to 16 bits
    constexpr ZeroSumTab() : blk{}, cdc{} {
        for (int q = 0; q < 52; ++q) {
            const int a = zero_sum_4x4_calc(q), b = zero_sum_chroma_dc_calc(q);
            blk[q] = (uint16_t)(a > 0xffff ? 0xffff : a);
            cdc[q] = (uint16_t)(b > 0xffff ? 0xffff : b);
        }
    }
};
// Largest sum |residual| of an inter 4x4 block (luma at the macroblock's qp, chroma AC at its qpc)
// for which every level is guaranteed 0.
MXHD int zero_sum_4x4(int qp) {
    constexpr ZeroSumTab tab;
    return tab.blk[qp < 0 ? 0 : (qp > 51 ? 51 : qp)];
}
// Largest sum |residual| of an inter 8x8 chroma plane for which its four DC levels are guaranteed 0.
MXHD int zero_sum_chroma_dc(int qpc) {
    constexpr ZeroSumTab tab;
    return tab.cdc[qpc < 0 ? 0 : (qpc > 51 ? 51 : qpc)];
}

// ME cost shared by both encoders.
MXHD uint32_t me_cost(uint32_t sad, int lambda, int mvx, int mvy) {
    return sad + (uint32_t)(lambda * (mvd_bits(mvx) + mvd_bits(mvy)));
}

// Integer search radius actually used: clamped to [4, 32] and rounded up to a multiple of
// 4 so the search window starts on a dword boundary.
MXHD int me_range(int r) {
    r = r < 4 ? 4 : (r > 32 ? 32 : r);
    return (r + 3) & ~3;
}
// Static-block early exit: a zero vector with SAD <= static_sad(qp) ends the search (both
// encoders apply the same rule, so their decisions stay bit-identical).  The reference is the
// lossy reconstruction, so an unchanged desktop region differs from it by the coding noise of
// the previous picture; a fixed threshold (128 = 0.5 per pixel) sent nearly every static MB of
// a QP-36 desktop through the full search (profiles/r02_c: ~1100 VALU per wave in k_me_full).
// A flat 16x16 residual of r per sample quantises to zero while r < ~qstep/4.7 (inter dead
// zone, 4x4 DC); 64 * lambda_sad(qp) ~ 256 * qstep / 12 stays well inside that.
constexpr uint32_t kStaticSad = 128;
MXHD uint32_t static_sad(int qp) {
    const uint32_t t = 64u * (uint32_t)lambda_sad(qp);
    return t > kStaticSad ? t : kStaticSad;
}

// ---- scroll hint (EncoderConfig::scroll_range): one axis-aligned displacement per P picture,
// found by a sparse 1-D probe, on which a macroblock may centre its +-R search instead of on zero.
// Every rule is here, once, for the probe kernel (k_scroll_probe), the search (me_full_body) and
// the CPU encoder (scroll_probe_cpu, me_search_cpu): the hint and the vectors stay bit-identical.
//
// Largest displacement looked for: [0, 192], rounded up to a multiple of 4 (the probe's strips are
// staged in whole dwords).  192 + 32 (largest me_range) + 1 (sub-sample refinement) stays inside
// the vertical vector range [-256, +255.75] of level 3.0, the lowest level pick_level() signals.
constexpr int kScrollMaxReach = 192;
MXHD int scroll_reach(int r) {
    r = r < 0 ? 0 : (r > kScrollMaxReach ? kScrollMaxReach : r);
    return (r + 3) & ~3;
}
// Probe macroblocks: every kScrollLattice-th macroblock in x and in y.
constexpr int kScrollLattice = 2;
MXHD bool scroll_is_probe(int mbx, int mby) { return mbx % kScrollLattice == 0 && mby % kScrollLattice == 0; }
MXHD int scroll_probes_x(int mb_w) { return (mb_w + kScrollLattice - 1) / kScrollLattice; }
MXHD int scroll_probes_y(int mb_h) { return (mb_h + kScrollLattice - 1) / kScrollLattice; }
// A hint needs this many probes voting for it, and at least half of all votes cast.
constexpr uint32_t kScrollMinVotes = 3;
// Histogram: bins [0, 2D] are the vertical displacements (0, d), bins [2D + 1, 4D + 1] the
// horizontal ones (d, 0), d = index - D.  The d = 0 bins are never voted for.
MXHD int scroll_bins(int D) { return 2 * (2 * D + 1); }
MXHD int scroll_bin(int axis, int d, int D) { return axis * (2 * D + 1) + d + D; }
// A probe's candidates are ordered by (SAD, |d|, axis (vertical first), index): the smallest key wins.
MXHD unsigned long long scroll_probe_key(uint32_t sad, int axis, int d, int D) {
    const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
    return ((unsigned long long)sad << 32) | (ad << 16) | (uint32_t)scroll_bin(axis, d, D);
}
// A probe whose best candidate has key k votes for bin scroll_key_bin(k) when scroll_key_votes(k, qp).
MXHD bool scroll_key_votes(unsigned long long k, int qp) { return (uint32_t)(k >> 32) <= static_sad(qp); }
MXHD int scroll_key_bin(unsigned long long k) { return (int)(k & 0xffffu); }
// The decision over the histogram: most votes, then the smaller |d|, then the vertical axis, then
// the negative displacement -- the LARGEST bin key wins.  A bin without votes has key 0.
MXHD unsigned long long scroll_bin_key(uint32_t votes, int bin, int D) {
    if (!votes) return 0ull;
    const int axis = bin / (2 * D + 1), d = bin % (2 * D + 1) - D;
    const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
    return ((unsigned long long)votes << 32) | ((0xfffu - ad) << 16) | ((uint32_t)(1 - axis) << 15) |
           ((uint32_t)(d < 0) << 14) | (uint32_t)bin;
}
// The hint (full samples) from the winning bin key and the number of votes cast; (0, 0): none.
MXHD void scroll_decide(unsigned long long best, uint32_t total, int D, int* gx, int* gy) {
    const uint32_t votes = (uint32_t)(best >> 32);
    *gx = *gy = 0;
    if (votes < kScrollMinVotes || 2u * votes < total) return;
    const int bin = (int)(best & 0x3fffu), axis = bin / (2 * D + 1), d = bin % (2 * D + 1) - D;
    if (axis) *gx = d; else *gy = d;
}
static_assert(2 * (2 * kScrollMaxReach + 1) < (1 << 14), "scroll_bin_key keeps the bin in 14 bits");
// What a macroblock whose zero vector failed the static exit does with a non-zero hint g:
// SADg within the static threshold -> it takes vector 4g (16x16) without a search; else the search
// is centred on g when SADg < SAD0, on zero otherwise.
enum ScrollUse : int { kScrollExit = 0, kScrollCentre = 1, kScrollZero = 2 };
MXHD int scroll_use(uint32_t sadg, uint32_t sad0, int qp) {
    return sadg <= static_sad(qp) ? kScrollExit : (sadg < sad0 ? kScrollCentre : kScrollZero);
}

// Sub-pel refinement neighbour k (0..7) offsets.
MXHD void subpel_offset(int k, int* dx, int* dy) {
    *dx = (k < 3) ? (k - 1) : (k == 3 ? -1 : (k == 4 ? 1 : (k - 6)));
    *dy = (k < 3) ? -1 : ((k == 3 || k == 4) ? 0 : 1);
}

}  // namespace h264
}  // namespace mx
