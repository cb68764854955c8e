// The root position of a search tree: the board geometry, the cell codes, the RootMeta record and the pure rules of its
// writers, stated once (DESIGN.md 3 "Root positions").  No HIP and nothing from search.hip: tests/test_root_position_host.py
// compiles it alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tg_root {

// a board of S x S points inside a border of one cell: W cells a row, NC cells, P points, A actions (PASS last), HMAX
// moves of record (board/constant.py:31)
template <int S>
struct Geo {
    static constexpr int W = S + 2;
    static constexpr int NC = W * W;
    static constexpr int P = S * S;
    static constexpr int A = P + 1;
    static constexpr int HMAX = 3 * P;
};

constexpr int kEmpty = 0, kBlack = 1, kWhite = 2, kOob = 3;      // cell codes; kBlack / kWhite: the colours as well
constexpr int kPass = 0;

// what a tree keeps of its root besides root_cells [NC] and root_hist [HMAX]
struct RootMeta {
    uint64_t hash;
    int32_t moves, ko_pos, ko_move, prev, prevprev, to_move;
    int32_t num_nodes;
    int32_t hist_len;   // number of valid history slots (== moves, clamped)
};
static_assert(sizeof(RootMeta) == 40 && offsetof(RootMeta, moves) == 8 && offsetof(RootMeta, hist_len) == 36,
              "tg_search_reroot and the read-outs copy the record as it is");

// history words a root carries: every recorded position where the board keeps them for superko, else one
constexpr int root_hist_len(int moves, int hmax, bool keeps_history) { return keeps_history ? (moves < hmax ? moves : hmax) : 1; }

// cell p of the empty board of width W: the border, or an empty point
constexpr int empty_board_cell(int p, int W) {
    const int x = p % W, y = p / W;
    return (x == 0 || y == 0 || x == W - 1 || y == W - 1) ? kOob : kEmpty;
}

// The root record of a position from its board scalars {hash, moves, ko_pos, ko_move, prev, prevprev}: no tree yet.
template <class Scalars>
constexpr RootMeta root_meta(const Scalars &b, int to_move, int hist_len) {
    return RootMeta{b.hash, b.moves, b.ko_pos, b.ko_move, b.prev, b.prevprev, to_move, /* num_nodes */ 0, hist_len};
}

// ---- replaying a game record (moves: padded coordinates, kPass = pass) from the empty board ----
// a record the host board has no move record for (board/constant.py:31): nothing of it is replayed
constexpr bool record_too_long(int64_t n_moves, int hmax) { return n_moves > hmax; }

// a move put_stone is specified for: a pass, or a coordinate of this board whose cell (cells[mv]) is empty
template <class Cells>
constexpr bool record_move_playable(int mv, int nc, const Cells &cells) {
    return mv == kPass || (mv > 0 && mv < nc && cells[mv] == kEmpty);
}

// The side to move before move `ply` of a record of n_moves (mcts/record_roots.py to_move_at): that move's colour -
// colors[ply], alternating from black without colours - and at the final position (ply == n_moves) GoBoard.get_to_move:
// the opponent of the last move's colour, black for an empty record.
constexpr int record_move_color(const int8_t *colors, int64_t ply) { return colors ? (int)colors[ply] : (ply & 1 ? kWhite : kBlack); }
constexpr int record_to_move(const int8_t *colors, int64_t n_moves, int64_t ply) {
    return ply < n_moves ? record_move_color(colors, ply) : n_moves == 0 ? kBlack : 3 - record_move_color(colors, n_moves - 1);
}

}  // namespace tg_root
