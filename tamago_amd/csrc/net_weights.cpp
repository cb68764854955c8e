// The weight images of the DualNet forward kernels (net_weights.h).  Host code only.
#include "net_weights.h"

#include <cstring>

namespace tg {

uint16_t f32_to_f16_rn(float f) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    const int32_t e = (int32_t)((x >> 23) & 0xFF) - 127 + 15;
    uint32_t man = x & 0x7FFFFFu;
    if (((x >> 23) & 0xFF) == 0xFF) return (uint16_t)(sign | 0x7C00u | (man ? 0x200u : 0));
    if (e >= 31) return (uint16_t)(sign | 0x7C00u);
    if (e <= 0) {
        if (e < -10) return (uint16_t)sign;
        man |= 0x800000u;
        const int shift = 14 - e;                              // 14 .. 24
        uint32_t h = man >> shift;
        const uint32_t rem = man & ((1u << shift) - 1), half = 1u << (shift - 1);
        if (rem > half || (rem == half && (h & 1))) ++h;
        return (uint16_t)(sign | h);
    }
    uint32_t h = ((uint32_t)e << 10) | (man >> 13);
    const uint32_t rem = man & 0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1))) ++h;     // may carry into the exponent: still right
    return (uint16_t)(sign | h);
}

float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    const uint32_t e = (h >> 10) & 0x1F, man = h & 0x3FFu;
    float out;
    if (e == 0) {
        out = std::ldexp((float)man, -24);
        uint32_t b;
        std::memcpy(&b, &out, 4);
        b |= sign;
        std::memcpy(&out, &b, 4);
        return out;
    }
    const uint32_t b = sign | ((e == 31 ? 0xFFu : e - 15 + 127) << 23) | (man << 13);
    std::memcpy(&out, &b, 4);
    return out;
}

void split_weight(float w, uint16_t *out) {
    const uint16_t h = f32_to_f16_rn(w);
    out[0] = h;
    out[1] = f32_to_f16_rn((w - f16_to_f32(h)) * 2048.f);
}

void split_pieces_scaled(double v, uint16_t *hi, uint16_t *lo) {
    const uint16_t h = f32_to_f16_rn((float)v);
    *hi = h;
    *lo = f32_to_f16_rn((float)((v - (double)f16_to_f32(h)) * 2048.0));
}

void split_pieces(double v, uint16_t *hi, uint16_t *lo) {
    const uint16_t h = f32_to_f16_rn((float)v);
    *hi = h;
    *lo = f32_to_f16_rn((float)(v - (double)f16_to_f32(h)));
}

int scale_exponent(double mx, int clamp) {
    int e = 0;
    if (mx > 0.0 && std::isfinite(mx)) {
        int ex;
        std::frexp(mx, &ex);                                   // mx = f * 2^ex, f in [0.5, 1)
        e = 10 - ex;
    }
    return e > clamp ? clamp : (e < -clamp ? -clamp : e);
}

void fold_bn(const float *w, const float *b, const float *mean, const float *var, int c, double eps, float *scale, float *shift) {
    for (int i = 0; i < c; ++i) {
        const double s = (double)w[i] / std::sqrt((double)var[i] + eps);
        scale[i] = (float)s;
        shift[i] = (float)((double)b[i] - (double)mean[i] * s);
    }
}

ExactImages exact_images(const float *blob, const ParamLayout &L, int board_size) {
    const int P = board_size * board_size, A = P + 1;
    auto vec = [&](size_t at, size_t n) { return std::vector<float>(blob + at, blob + at + n); };
    ExactImages im;
    im.scale.resize(kConvLayers * 64);
    im.shift.resize(kConvLayers * 64);
    for (int l = 0; l < kConvLayers; ++l)
        fold_bn(blob + L.bn_w[l], blob + L.bn_b[l], blob + L.bn_m[l], blob + L.bn_v[l], 64, bn_eps(l), &im.scale[l * 64], &im.shift[l * 64]);
    // stem: conv_layer.weight [64][6][3][3] -> w0frag[w][tap][lane][2]
    im.w0frag.assign(4 * 9 * 64 * 2, 0.f);
    {
        const float *w = blob + L.conv[0];
        for (int wv = 0; wv < 4; ++wv)
            for (int tap = 0; tap < 9; ++tap)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 2; ++j) {
                        const int n = lane & 15, g = lane >> 4, cin = 4 * j + g, cout = 16 * wv + n;
                        const float v = cin < 6 ? w[(cout * 6 + cin) * 9 + tap] : 0.f;
                        im.w0frag[((wv * 9 + tap) * 64 + lane) * 2 + j] = v;
                    }
    }
    // tower: layer 0..11 of the images = layer 1..12 of the blob
    im.wfrag.resize((size_t)kTowerLayers * 4 * 9 * 4 * 64 * 4);
    im.wwino.resize((size_t)kTowerLayers * 4 * 16 * 4 * 64 * 4);
    for (int layer = 0; layer < kTowerLayers; ++layer) {
        const float *w = blob + L.conv[1 + layer];
        for (int wv = 0; wv < 4; ++wv)
            for (int tap = 0; tap < 9; ++tap)
                for (int s = 0; s < 4; ++s)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 4; ++j) {
                            const int n = lane & 15, g = lane >> 4;
                            const int cin = 16 * s + 4 * g + j, cout = 16 * wv + n;
                            im.wfrag[(((((size_t)layer * 4 + wv) * 9 + tap) * 4 + s) * 64 + lane) * 4 + j] = w[(cout * 64 + cin) * 9 + tap];
                        }
        // Winograd F(2x2,3x3) weights U = G g G^T, G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]
        for (int cout = 0; cout < 64; ++cout)
            for (int cin = 0; cin < 64; ++cin) {
                const float *g = &w[(cout * 64 + cin) * 9];
                double gg[4][3], u[4][4];
                for (int k = 0; k < 3; ++k) {
                    gg[0][k] = g[k];
                    gg[1][k] = 0.5 * ((double)g[k] + g[3 + k] + g[6 + k]);
                    gg[2][k] = 0.5 * ((double)g[k] - g[3 + k] + g[6 + k]);
                    gg[3][k] = g[6 + k];
                }
                for (int a = 0; a < 4; ++a) {
                    u[a][0] = gg[a][0];
                    u[a][1] = 0.5 * (gg[a][0] + gg[a][1] + gg[a][2]);
                    u[a][2] = 0.5 * (gg[a][0] - gg[a][1] + gg[a][2]);
                    u[a][3] = gg[a][2];
                }
                const int wv = cout / 16, n = cout % 16, sgrp = cin / 16, gq = (cin % 16) / 4, j = cin % 4;
                const int lane = gq * 16 + n;
                for (int xi = 0; xi < 16; ++xi)
                    im.wwino[(((((size_t)layer * 4 + wv) * 4 + sgrp) * 16 + xi) * 64 + lane) * 4 + j] = (float)u[xi / 4][xi % 4];
            }
    }
    // heads
    im.hp_w = vec(L.p_conv, 2 * 64);
    im.hv_w = vec(L.v_conv, 64);
    im.head_ss.resize(6);           // policy scale0, shift0, scale1, shift1, value scale, shift
    {
        float sc[2], sh[2];
        fold_bn(blob + L.p_bn_w, blob + L.p_bn_b, blob + L.p_bn_m, blob + L.p_bn_v, 2, kBnEps, sc, sh);
        im.head_ss[0] = sc[0]; im.head_ss[1] = sh[0]; im.head_ss[2] = sc[1]; im.head_ss[3] = sh[1];
    }
    fold_bn(blob + L.v_bn_w, blob + L.v_bn_b, blob + L.v_bn_m, blob + L.v_bn_v, 1, kBnEps, &im.head_ss[4], &im.head_ss[5]);
    // [A][2P] as the state_dict holds it -> [2P][A] (padded to whole 4 KB: the split-operand kernel copies it into LDS in 1 KB pieces)
    im.pfc_wT.assign((((size_t)2 * P * A * 4 + 4095) / 4096) * 1024, 0.f);
    const float *pfc = blob + L.p_fc_w;
    for (int a = 0; a < A; ++a)
        for (int j = 0; j < 2 * P; ++j) im.pfc_wT[(size_t)j * A + a] = pfc[(size_t)a * 2 * P + j];
    im.pfc_b = vec(L.p_fc_b, A);
    im.vfc_w = vec(L.v_fc_w, (size_t)3 * P);
    im.vfc_b = vec(L.v_fc_b, 3);
    return im;
}

SplitImage split_image(const float *blob, const ParamLayout &L, const std::vector<float> &scale) {
    constexpr int np = 2;                                      // pieces
    const size_t tap_bytes = (size_t)2 * np * 4 * 1024;
    SplitImage im;
    im.wsplit.assign((size_t)kSplitTaps * tap_bytes / 2, 0);
    im.sscale.resize(kConvLayers * 64);
    im.spread = 1.0;
    for (int layer = 0; layer <= kTowerLayers; ++layer) {
        ChannelSpread cs;
        const float *w = blob + L.conv[layer];
        const size_t n = layer == 0 ? kStemW : kTowerW;
        float mx = 0.f;
        for (size_t i = 0; i < n; ++i) mx = std::fmax(mx, std::fabs(w[i]));
        const int e = scale_exponent(mx, kNoClamp);
        const float up = std::ldexp(1.f, e), down = std::ldexp(1.f, -e);
        for (int i = 0; i < 64; ++i) im.sscale[layer * 64 + i] = scale[layer * 64 + i] * down;
        const int ntaps = layer == 0 ? 1 : 9;
        for (int tap = 0; tap < ntaps; ++tap) {
            const int g = layer == 0 ? 0 : 1 + (layer - 1) * 9 + tap;
            for (int kc = 0; kc < 2; ++kc)
                for (int ct = 0; ct < 4; ++ct)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int el = 0; el < 8; ++el) {
                            const FragAt at = frag_at(ct, kc, lane, el);       // row = output channel
                            const int k = at.k;
                            float v;
                            if (layer == 0) {                  // k = tap' * 6 + plane
                                const int t2 = k / 6, c2 = k % 6;
                                v = k < 54 ? w[(at.row * 6 + c2) * 9 + t2] : 0.f;
                            } else {
                                v = w[((size_t)at.row * 64 + k) * 9 + tap];
                            }
                            uint16_t pc[np];
                            split_weight(v * up, pc);
                            if (layer > 0) cs.add(k, v);
                            for (int p = 0; p < np; ++p)
                                im.wsplit[((((size_t)g * 2 + kc) * np + p) * 4 + ct) * 512 + lane * 8 + el] = pc[p];
                        }
        }
        im.spread = std::fmax(im.spread, cs.spread());
    }
    return im;
}

HeadsImages heads_images(const float *blob, const ParamLayout &L, int board_size, const std::vector<float> &head_ss) {
    const int P = board_size * board_size, A = P + 1, K = 2 * P;
    const float *hp_w = blob + L.p_conv, *hv_w = blob + L.v_conv, *pfc_w = blob + L.p_fc_w;
    HeadsImages im;
    // ---- 1x1 convolutions: channel 0 / 1 = policy, 2 = value, 3..15 = 0 ----
    auto w1 = [&](int ch, int k) -> double {
        if (ch == 0) return (double)hp_w[k] * head_ss[0];
        if (ch == 1) return (double)hp_w[64 + k] * head_ss[2];
        if (ch == 2) return (double)hv_w[k] * head_ss[4];
        return 0.0;
    };
    double mx = 0.0;
    for (int ch = 0; ch < 3; ++ch)
        for (int k = 0; k < 64; ++k) mx = std::fmax(mx, std::fabs(w1(ch, k)));
    const int e1 = scale_exponent(mx, kExpClamp);
    im.hd1_img.assign((size_t)2 * 2 * 512, 0);                 // [kc][piece][lane][8]
    for (int kc = 0; kc < 2; ++kc)
        for (int lane = 0; lane < 64; ++lane)
            for (int el = 0; el < 8; ++el) {
                const FragAt at = frag_at(0, kc, lane, el);    // row = head channel
                const size_t base = ((size_t)kc * 2) * 512 + lane * 8 + el;
                split_pieces_scaled(w1(at.row, at.k) * std::ldexp(1.0, e1), &im.hd1_img[base], &im.hd1_img[base + 512]);
            }
    im.hd1_tab.assign(20, 0.f);
    im.hd1_tab[0] = (float)((double)head_ss[1] * std::ldexp(1.0, e1));
    im.hd1_tab[1] = (float)((double)head_ss[3] * std::ldexp(1.0, e1));
    im.hd1_tab[2] = (float)((double)head_ss[5] * std::ldexp(1.0, e1));
    im.hd1_tab[16] = std::ldexp(1.f, -e1);
    // ---- policy FC: logits[a] = sum_k W[a][k] h[k] + bias[a], k = channel * P + position ----
    constexpr int NT = kHeadsNT, KS = kHeadsKS;
    mx = 0.0;
    for (size_t i = 0; i < (size_t)A * K; ++i) mx = std::fmax(mx, std::fabs((double)pfc_w[i]));
    const int e2 = scale_exponent(mx, kExpClamp);
    im.pfc_img.assign((size_t)NT * KS * 2 * 512, 0);           // [nt][ks][piece][lane][8]
    for (int nt = 0; nt < NT; ++nt)
        for (int ks = 0; ks < KS; ++ks)
            for (int lane = 0; lane < 64; ++lane)
                for (int el = 0; el < 8; ++el) {
                    const FragAt at = frag_at(nt, ks, lane, el);               // row = action
                    const int a = at.row, k = at.k;
                    const double v = (a < A && k < K) ? (double)pfc_w[(size_t)a * K + k] * std::ldexp(1.0, e2) : 0.0;
                    const size_t base = ((size_t)(nt * KS + ks) * 2) * 512 + lane * 8 + el;
                    split_pieces_scaled(v, &im.pfc_img[base], &im.pfc_img[base + 512]);
                }
    im.pfc_tab.assign(4, 0.f);
    im.pfc_tab[0] = std::ldexp(1.f, -e2);
    return im;
}

W1dImage w1d_image(const float *blob, const ParamLayout &L, const std::vector<float> &scale, const std::vector<float> &shift) {
    W1dImage im;
    im.w1_w.resize((size_t)kTowerLayers * 4 * 3 * 2 * 2 * 4 * 512);
    im.w1_down.resize(kTowerLayers);
    im.w1_shift.resize(kTowerLayers * 64);
    im.spread = 1.0;
    std::vector<double> u((size_t)4 * 3 * 64 * 64);
    for (int layer = 0; layer < kTowerLayers; ++layer) {
        ChannelSpread cs;
        const float *w = blob + L.conv[1 + layer];
        double mx = 0.0;
        for (int cout = 0; cout < 64; ++cout)
            for (int cin = 0; cin < 64; ++cin) {
                const float *g = &w[((size_t)cout * 64 + cin) * 9];
                const double sc = scale[(layer + 1) * 64 + cout];
                for (int ky = 0; ky < 3; ++ky) {
                    const double g0 = g[ky * 3], g1 = g[ky * 3 + 1], g2 = g[ky * 3 + 2];
                    const double pt[4] = {g0, 0.5 * (g0 + g1 + g2), 0.5 * (g0 - g1 + g2), g2};
                    for (int p = 0; p < 4; ++p) {
                        const double v = pt[p] * sc;
                        u[(((size_t)p * 3 + ky) * 64 + cin) * 64 + cout] = v;
                        mx = std::fmax(mx, std::fabs(v));
                    }
                }
            }
        const int e = scale_exponent(mx, kExpClamp);
        im.w1_down[layer] = std::ldexp(1.f, -e);
        for (int c = 0; c < 64; ++c) im.w1_shift[layer * 64 + c] = shift[(layer + 1) * 64 + c];
        for (int p = 0; p < 4; ++p)
            for (int ky = 0; ky < 3; ++ky)
                for (int kc = 0; kc < 2; ++kc)
                    for (int ct = 0; ct < 4; ++ct)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int el = 0; el < 8; ++el) {
                                const FragAt at = frag_at(ct, kc, lane, el);   // row = output channel, k = input channel
                                const double v = std::ldexp(u[(((size_t)p * 3 + ky) * 64 + at.k) * 64 + at.row], e);
                                const size_t frag = ((((size_t)layer * 4 + p) * 3 + ky) * 2 + kc) * 2;
                                split_pieces(v, &im.w1_w[((frag + 0) * 4 + ct) * 512 + lane * 8 + el],
                                             &im.w1_w[((frag + 1) * 4 + ct) * 512 + lane * 8 + el]);
                                cs.add(at.k, v);
                            }
        im.spread = std::fmax(im.spread, cs.spread());
    }
    return im;
}

}  // namespace tg
