// The DualNet parameter blob: WHICH tensors it holds, in which order, stated once (DESIGN.md 3 "Parameter blob and weight
// images").  tg_net_param_count, tg_net_create (through net_weights.cpp) and the training step (train.hip, whose kernels get the
// layout by value) all read this layout; Python's state_dict_keys (nn/network/dual_net.py) names the same tensors in the same
// order, and tests/test_net_weights_host.py holds the two against each other offset by offset.  No HIP: the host compiler
// builds it alone.
#pragma once
#include <cstddef>

namespace tg {

constexpr int kBlocks = 6;                    // residual blocks
constexpr int kConvLayers = 1 + 2 * kBlocks;  // 13: stem + two per block
constexpr int kFilters = 64, kPlanes = 6;
constexpr size_t kStemW = (size_t)kFilters * kPlanes * 9, kTowerW = (size_t)kFilters * kFilters * 9;

// Batch norm: epsilon and the momentum of the running statistics - the stem is a default nn.BatchNorm2d, every other one
// (blocks, heads) is built with eps 2e-5, momentum 0.01
constexpr double kBnEpsStem = 1e-5, kBnEps = 2e-5;
constexpr float kBnMomentumStem = 0.1f, kBnMomentum = 0.01f;
constexpr double bn_eps(int layer) { return layer == 0 ? kBnEpsStem : kBnEps; }

// offsets in floats; layer l: 0 = stem, 1 + 2b / 2 + 2b = conv1 / conv2 of block b.  bn_*: weight, bias, running mean, running var
struct ParamLayout {
    size_t conv[kConvLayers], bn_w[kConvLayers], bn_b[kConvLayers], bn_m[kConvLayers], bn_v[kConvLayers];
    size_t p_conv, p_bn_w, p_bn_b, p_bn_m, p_bn_v, p_fc_w, p_fc_b;
    size_t v_conv, v_bn_w, v_bn_b, v_bn_m, v_bn_v, v_fc_w, v_fc_b;
    size_t total;
};

inline ParamLayout make_layout(int S) {
    const size_t P = (size_t)S * S, A = P + 1;
    ParamLayout L{};
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o += n; return r; };
    auto bn = [&](int l) { L.bn_w[l] = take(kFilters); L.bn_b[l] = take(kFilters); L.bn_m[l] = take(kFilters); L.bn_v[l] = take(kFilters); };
    L.conv[0] = take(kStemW);
    bn(0);
    for (int b = 0; b < kBlocks; ++b) {
        L.conv[1 + 2 * b] = take(kTowerW);
        L.conv[2 + 2 * b] = take(kTowerW);
        bn(1 + 2 * b);
        bn(2 + 2 * b);
    }
    L.p_conv = take(2 * kFilters); L.p_bn_w = take(2); L.p_bn_b = take(2); L.p_bn_m = take(2); L.p_bn_v = take(2);
    L.p_fc_w = take(A * 2 * P); L.p_fc_b = take(A);
    L.v_conv = take(kFilters); L.v_bn_w = take(1); L.v_bn_b = take(1); L.v_bn_m = take(1); L.v_bn_v = take(1);
    L.v_fc_w = take(3 * P); L.v_fc_b = take(3);
    L.total = o;
    return L;
}

}  // namespace tg
