// Every weight image of the DualNet forward kernels, built on the host from the parameter blob (net_params.h): pure functions
// from (blob, layout) to plain vectors, one per kernel family.  tg_net_create and the *_prepare functions of the forward
// translation units upload what these return and point NetDev (net_device.h, which documents each image's index order) at
// it.  No HIP: tests/test_net_weights_host.py compiles net_weights.cpp alone and holds every image to recorded bits.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "net_params.h"

namespace tg {

constexpr int kTowerLayers = 2 * kBlocks;             // 12
constexpr int kSplitTaps = 1 + 9 * kTowerLayers;      // split image: stem as one K = 64 pseudo-tap + 12 x 9
constexpr int kHeadsNT = 6, kHeadsKS = 6;             // policy-FC fragment image: 16-action tiles, 32-feature steps (9x9)

// ---- number formats ------------------------------------------------------------------------------------------------
uint16_t f32_to_f16_rn(float f);                      // round to nearest even; a NaN stays a (quiet) NaN
float f16_to_f32(uint16_t h);

// Two f16 pieces of an (already scaled) weight - three arithmetics, three sets of bits, each the one its kernel family was
// measured with: split_weight (split image) subtracts in fp32, low piece x 2048; split_pieces_scaled (head images) in fp64,
// low piece x 2048; split_pieces (w1d image) in fp64, low piece unscaled.
void split_weight(float w, uint16_t *out);
void split_pieces_scaled(double v, uint16_t *hi, uint16_t *lo);
void split_pieces(double v, uint16_t *hi, uint16_t *lo);

// The power of two that takes an image's largest entry `mx` into [2^9, 2^10): the exponent e (0 for mx = 0 or not finite),
// held to +-clamp.  The head and w1d images clamp to kExpClamp, the split image does not (kNoClamp).
constexpr int kExpClamp = 40, kNoClamp = 1 << 20;
int scale_exponent(double mx, int clamp);

// A fragment of the 16x16x32 f16 MFMA as a wave loads it ([lane 64][8 x 16 bit]): element `el` of lane `lane` in row tile
// `tile`, k-chunk `chunk` is entry (row, k) of the matrix
struct FragAt { int row, k; };
inline FragAt frag_at(int tile, int chunk, int lane, int el) { return {tile * 16 + (lane & 15), chunk * 32 + (lane >> 4) * 8 + el}; }

// scale = w / sqrt(var + eps), shift = b - mean * scale, in fp64, of `c` channels
void fold_bn(const float *w, const float *b, const float *mean, const float *var, int c, double eps, float *scale, float *shift);

// Spread of a tower layer's input channels: the largest weight (over outputs and taps) of each input channel, the largest of
// the 64 over the smallest that is not zero.  A weight image has ONE power-of-two scaling per layer and the activations none per
// channel: an input channel whose weights are 2^S times another's is one whose activations are expected 2^S times smaller -
// their low f16 piece sinks below the subnormal quantum 2^-24 - while the other's weights keep S bits fewer.  About 1 for
// weights of one magnitude; what the load-time guard of the f16 towers looks at (tg_net_channel_spread, net_forward.hip).
struct ChannelSpread {
    double mx[64] = {};
    void add(int cin, double v) {
        const double a = std::fabs(v);
        if (a > mx[cin]) mx[cin] = a;                          // (a NaN is never larger)
    }
    double spread() const {
        double hi = 0.0, lo = INFINITY;
        for (int c = 0; c < 64; ++c)
            if (mx[c] > 0.0) {
                if (mx[c] > hi) hi = mx[c];
                if (mx[c] < lo) lo = mx[c];
            }
        return hi > 0.0 ? hi / lo : 1.0;
    }
};

// ---- the images, named like the NetDev members they become ----------------------------------------------------------
// exact-fp32 kernels: fragment-ordered convolution weights (direct and Winograd G g G^T), folded batch norm, fp32 heads
struct ExactImages {
    std::vector<float> w0frag, wfrag, wwino, scale, shift, hp_w, hv_w, head_ss, pfc_wT, pfc_b, vfc_w, vfc_b;
};
ExactImages exact_images(const float *blob, const ParamLayout &L, int board_size);

// direct split-operand kernels: f16 x 2 pieces, x 2^e per layer (not clamped); sscale = folded scale x 2^-e
struct SplitImage {
    std::vector<uint16_t> wsplit;
    std::vector<float> sscale;
    double spread;
};
SplitImage split_image(const float *blob, const ParamLayout &L, const std::vector<float> &scale);

// 9x9 head phase on the f16 matrix pipe: the 1x1 convolutions (batch norm folded: scale into the weights in fp64, shift ->
// accumulator start) and the policy FC, both as f16 x 2 pieces with a power-of-two scaling per image
struct HeadsImages {
    std::vector<uint16_t> hd1_img, pfc_img;
    std::vector<float> hd1_tab, pfc_tab;
};
HeadsImages heads_images(const float *blob, const ParamLayout &L, int board_size, const std::vector<float> &head_ss);

// one-axis Winograd kernels: U_p[ky] = (G g[ky])_p along kx in fp64 with the batch-norm scale folded in, x 2^e per layer,
// low pieces unscaled; folded shift [12][64]; 2^-e [12]
struct W1dImage {
    std::vector<uint16_t> w1_w;
    std::vector<float> w1_shift, w1_down;
    double spread;
};
W1dImage w1d_image(const float *blob, const ParamLayout &L, const std::vector<float> &scale, const std::vector<float> &shift);

}  // namespace tg
