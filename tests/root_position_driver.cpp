// Stand-alone driver of csrc/root_position.h for tests/test_root_position_host.py (host compiler, no HIP): every rule the
// header owns, one fact per line, at 9x9, 13x13 and 19x19 - the geometry, the RootMeta layout and its fill, the empty board's
// cells, the history length, the replay's move check and the side to move at every ply of three records.
#include <cstddef>
#include <cstdio>
#include <vector>

#include "../tamago_amd/csrc/root_position.h"

using namespace tg_root;

struct Scalars {
    uint64_t hash;
    int moves, ko_pos, ko_move, prev, prevprev;
};

static void to_move_rows(int S, const char *name, const std::vector<int8_t> &colors, bool tagged) {
    const int64_t n = (int64_t)colors.size();
    printf("to_move %d %s", S, name);
    for (int64_t ply = 0; ply <= n; ++ply) printf(" %d", record_to_move(tagged ? colors.data() : nullptr, n, ply));
    printf("\n");
}

template <int S>
static void board_size() {
    using G = Geo<S>;
    printf("geo %d %d %d %d %d %d\n", S, G::W, G::NC, G::P, G::A, G::HMAX);
    std::vector<uint8_t> cells(G::NC);
    printf("cells %d", S);
    for (int p = 0; p < G::NC; ++p) printf(" %d", cells[p] = (uint8_t)empty_board_cell(p, G::W));
    printf("\n");
    for (int keeps = 0; keeps < 2; ++keeps)
        for (int moves : {1, 2, G::HMAX - 1, G::HMAX, G::HMAX + 1})
            printf("hist_len %d %d %d %d\n", S, moves, keeps, root_hist_len(moves, G::HMAX, keeps != 0));
    for (int n : {0, G::HMAX - 1, G::HMAX, G::HMAX + 1}) printf("too_long %d %d %d\n", S, n, (int)record_too_long(n, G::HMAX));
    const int empty = 2 * G::W + 3, occupied = 3 * G::W + 2, border = 4 * G::W;
    cells[occupied] = kWhite;
    const struct { const char *name; int mv; } probes[] = {{"pass", kPass}, {"negative", -1}, {"beyond", G::NC}, {"last_cell", G::NC - 1},
                                                           {"empty", empty}, {"occupied", occupied}, {"border", border}};
    for (const auto &probe : probes) printf("playable %d %s %d %d\n", S, probe.name, probe.mv, (int)record_move_playable(probe.mv, G::NC, cells));
    to_move_rows(S, "empty", {}, false);
    to_move_rows(S, "alternating", std::vector<int8_t>(5, 0), false);
    to_move_rows(S, "tagged", {kBlack, kWhite, kWhite, kBlack, kWhite, kWhite}, true);
    to_move_rows(S, "white_first", {kWhite, kBlack, kWhite}, true);
    const Scalars b{0x0123456789abcdefull + S, 7, 30, 5, 41, 0};
    const RootMeta m = root_meta(b, kWhite, 3);
    printf("fill %d %llu %d %d %d %d %d %d %d %d\n", S, (unsigned long long)m.hash, m.moves, m.ko_pos, m.ko_move, m.prev, m.prevprev,
           m.to_move, m.num_nodes, m.hist_len);
}

int main() {
    printf("codes %d %d %d %d %d\n", kEmpty, kBlack, kWhite, kOob, kPass);
    printf("meta %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(RootMeta), offsetof(RootMeta, hash), offsetof(RootMeta, moves),
           offsetof(RootMeta, ko_pos), offsetof(RootMeta, ko_move), offsetof(RootMeta, prev), offsetof(RootMeta, prevprev),
           offsetof(RootMeta, to_move), offsetof(RootMeta, num_nodes), offsetof(RootMeta, hist_len));
    board_size<9>();
    board_size<13>();
    board_size<19>();
    return 0;
}
