// Host driver of csrc/net_params.h + csrc/net_weights.cpp for tests/test_net_weights_host.py (no HIP, no GPU).
//   driver <board size> <blob: raw float32> <out dir>   prints the blob layout and both channel spreads, writes every weight
//                                                       image as <out dir>/<NetDev member>.bin
//   driver f16 <values: raw float32> <out dir>          writes f16_to_f32 of all 65536 bit patterns (f16_to_f32.bin) and
//                                                       f32_to_f16_rn of the values (f32_to_f16.bin)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../tamago_amd/csrc/net_weights.h"

namespace {

template <typename T>
std::vector<T> read_all(const char *path) {
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::perror(path); std::exit(2); }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) { std::perror(path); std::exit(2); }
    std::fclose(f);
    return v;
}

template <typename T>
void write_all(const std::string &dir, const char *name, const std::vector<T> &v) {
    const std::string path = dir + "/" + name + ".bin";
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { std::perror(path.c_str()); std::exit(2); }
    std::fclose(f);
}

// (tensor name as Python's state_dict_keys spells it, offset): written out member by member, then sorted by offset - a
// tensor's count is the distance to the next one
void print_layout(const tg::ParamLayout &L) {
    std::vector<std::pair<size_t, std::string>> rows;
    auto bn = [&](const std::string &prefix, size_t w, size_t b, size_t m, size_t v) {
        rows.push_back({w, prefix + ".weight"});
        rows.push_back({b, prefix + ".bias"});
        rows.push_back({m, prefix + ".running_mean"});
        rows.push_back({v, prefix + ".running_var"});
    };
    rows.push_back({L.conv[0], "conv_layer.weight"});
    bn("bn_layer", L.bn_w[0], L.bn_b[0], L.bn_m[0], L.bn_v[0]);
    for (int b = 0; b < tg::kBlocks; ++b)
        for (int c = 1; c <= 2; ++c) {
            const int l = 2 * b + c;
            const std::string blk = "blocks." + std::to_string(b);
            rows.push_back({L.conv[l], blk + ".conv" + std::to_string(c) + ".weight"});
            bn(blk + ".bn" + std::to_string(c), L.bn_w[l], L.bn_b[l], L.bn_m[l], L.bn_v[l]);
        }
    rows.push_back({L.p_conv, "policy_head.conv_layer.weight"});
    bn("policy_head.bn_layer", L.p_bn_w, L.p_bn_b, L.p_bn_m, L.p_bn_v);
    rows.push_back({L.p_fc_w, "policy_head.fc_layer.weight"});
    rows.push_back({L.p_fc_b, "policy_head.fc_layer.bias"});
    rows.push_back({L.v_conv, "value_head.conv_layer.weight"});
    bn("value_head.bn_layer", L.v_bn_w, L.v_bn_b, L.v_bn_m, L.v_bn_v);
    rows.push_back({L.v_fc_w, "value_head.fc_layer.weight"});
    rows.push_back({L.v_fc_b, "value_head.fc_layer.bias"});
    std::sort(rows.begin(), rows.end());
    for (size_t i = 0; i < rows.size(); ++i)
        std::printf("layout %s %zu %zu\n", rows[i].second.c_str(), rows[i].first,
                    (i + 1 < rows.size() ? rows[i + 1].first : L.total) - rows[i].first);
    std::printf("total %zu\n", L.total);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const std::string dir = argv[3];
    if (!std::strcmp(argv[1], "f16")) {
        std::vector<float> widened(65536);
        for (int h = 0; h < 65536; ++h) widened[h] = tg::f16_to_f32((uint16_t)h);
        write_all(dir, "f16_to_f32", widened);
        const std::vector<float> values = read_all<float>(argv[2]);
        std::vector<uint16_t> narrowed(values.size());
        for (size_t i = 0; i < values.size(); ++i) narrowed[i] = tg::f32_to_f16_rn(values[i]);
        write_all(dir, "f32_to_f16", narrowed);
        return 0;
    }
    const int S = std::atoi(argv[1]);
    const tg::ParamLayout L = tg::make_layout(S);
    print_layout(L);
    const std::vector<float> blob = read_all<float>(argv[2]);
    if (blob.size() != L.total) { std::fprintf(stderr, "blob: %zu floats, layout: %zu\n", blob.size(), L.total); return 2; }
    const tg::ExactImages ex = tg::exact_images(blob.data(), L, S);
    write_all(dir, "w0frag", ex.w0frag); write_all(dir, "wfrag", ex.wfrag); write_all(dir, "wwino", ex.wwino);
    write_all(dir, "scale", ex.scale); write_all(dir, "shift", ex.shift);
    write_all(dir, "hp_w", ex.hp_w); write_all(dir, "hv_w", ex.hv_w); write_all(dir, "head_ss", ex.head_ss);
    write_all(dir, "pfc_wT", ex.pfc_wT); write_all(dir, "pfc_b", ex.pfc_b);
    write_all(dir, "vfc_w", ex.vfc_w); write_all(dir, "vfc_b", ex.vfc_b);
    const tg::SplitImage sp = tg::split_image(blob.data(), L, ex.scale);
    write_all(dir, "wsplit", sp.wsplit); write_all(dir, "sscale", sp.sscale);
    if (S == 9) {                                   // (the f16 head phase is the 9x9 kernels')
        const tg::HeadsImages hd = tg::heads_images(blob.data(), L, S, ex.head_ss);
        write_all(dir, "hd1_img", hd.hd1_img); write_all(dir, "hd1_tab", hd.hd1_tab);
        write_all(dir, "pfc_img", hd.pfc_img); write_all(dir, "pfc_tab", hd.pfc_tab);
    }
    const tg::W1dImage w1 = tg::w1d_image(blob.data(), L, ex.scale, ex.shift);
    write_all(dir, "w1_w", w1.w1_w); write_all(dir, "w1_shift", w1.w1_shift); write_all(dir, "w1_down", w1.w1_down);
    std::printf("spread split %a\nspread w1d %a\n", sp.spread, w1.spread);
    return 0;
}
