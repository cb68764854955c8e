"""Position corpus for the device board rules (put_stone / gen_candidates of csrc/search.hip) - CPU only, deterministic.

An entry is (size, moves, to_move, name): `moves` are padded coordinates played from the empty board with colours strictly
alternating from black (0 = PASS) - what tg_search_play can reproduce - and `to_move` is the colour that follows.  Sources:

* seeded fights: uniform play over the legal points that are no complete eye of the mover, 3 % passes, sampled every few plies;
* ko forks: every position of such a game right after a move that set the ko point (the retake is forbidden by the ko rule) and
  the same record followed by two passes (the ko rule has expired, the retake is forbidden by superko alone);
* crafted records for what random play does not deliver (CRAFTED below, each verified by the point it expects);
* history limit: a ko fork padded with leading passes so that GoBoard.moves at the root is HMAX - 2 .. HMAX + 4.

coverage() counts, with the oracle board, what the corpus holds per category; MINIMUMS are asserted by
tests/test_rule_corpus_host.py.  The comparison code of the GPU tests (check_roots, walk_tree, check_leaves) lives here too,
behind a small reader interface, so that the CPU suite can prove that it discriminates (OracleReader + PERTURBATIONS)."""
import functools
import os
import sys
from collections import Counter, namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.board import BLACK, EMPTY, OUT_OF_BOARD, PASS, WHITE, GoBoard, opponent  # noqa: E402

Entry = namedtuple("Entry", "size moves to_move name")

SIZES = (9, 13, 19)
# (sampled games, plies per game, sampling step, ko forks kept, games searched for ko forks) per size: within 512 / 160 / 96
# positions
PLAN = {9: (7, 300, 5, 6, 7), 13: (2, 500, 10, 6, 10), 19: (2, 600, 20, 6, 4)}
LIMITS = {9: 512, 13: 160, 19: 96}
SEED = {9: 9001, 13: 13001, 19: 19001}
PLAY_CAP_19 = 600          # longest record the device-play test replays at 19x19
HISTORY_OFFSETS = (-2, -1, 0, 2, 4)
N_TREE_ROOTS = {9: 16, 13: 6, 19: 16}

MINIMUMS = {"superko_only": 5, "ko": 5, "slow_kept": 3, "slow_pruned": 8, "slow_multi": 3, "complete_eye": 100,
            "incomplete_eye": 20, "suicide": 100, "multi_capture": 2, "capture_20": 2, "merge_3": 2, "ko_set": 2}


def hmax(size: int) -> int:
    return 3 * size * size


def color_after(moves) -> int:
    return BLACK if len(moves) % 2 == 0 else WHITE


def replay(entry, superko: bool = True, board_cls=GoBoard):
    board = board_cls(entry.size, 7.0, superko)
    color = BLACK
    for pos in entry.moves:
        board.put_stone(int(pos), color)
        color = opponent(color)
    assert color == entry.to_move
    return board


# ---- seeded fights ---------------------------------------------------------------------------------------------------------
def play_game(size: int, seed: int, plies: int):
    """(moves, plies after which the ko point was just set)."""
    board = GoBoard(size, 7.0, True)
    rs = np.random.RandomState(seed)
    color = BLACK
    moves, kos = [], []
    for ply in range(plies):
        legal = [p for p in board.get_all_legal_pos(color) if not board.is_complete_eye(p, color)]
        take_pass = rs.random_sample() < 0.03
        pos = PASS if (not legal or take_pass) else legal[rs.randint(len(legal))]
        board.put_stone(pos, color)
        moves.append(pos)
        if pos != PASS and board.ko_move == board.moves - 1:
            kos.append(ply + 1)
        color = opponent(color)
    return moves, kos


# ---- crafted records -------------------------------------------------------------------------------------------------------
# Diagrams sit in the top-left corner of the board (X black, O white, everything else empty); `tail` are the moves played
# after the stones stand, `mover` the colour to move at the entry's position and `expect` the (category, (x, y)) pairs that
# point_categories / move_categories must report there (1-based x, y from the top-left corner).
CRAFTED = [
    # two black strings of two liberties each, {p, (1,2)} and {p, (8,1)}: the union reaches three, the point stays
    dict(name="slow_kept", rows=["XXX.XXX.", ".OOOOOO."], mover=BLACK,
         expect=[("slow_kept", (4, 1)), ("slow_multi", (4, 1))]),
    # two black strings that share both liberties {(1,2), (2,2)}: self-atari of 7 stones at either point
    dict(name="slow_pruned_shared", rows=["XXXO", "..OO", "XXXO", "OOOO"], mover=BLACK,
         expect=[("slow_pruned", (1, 2)), ("slow_pruned", (2, 2)), ("slow_multi", (1, 2))]),
    # one string of 7 stones on three sides of (2,2) with liberties {(2,2), (4,1)}: pruned there, kept at (4,1)
    dict(name="slow_same_string_3_sides", rows=["XXX.", "X.OO", "XXXO", "OOOO"], mover=BLACK,
         expect=[("slow_pruned", (2, 2)), ("slow_kept", (4, 1)), ("same_string_twice", (2, 2))]),
    # one string of 6 stones above and left of (2,2) with liberties {(2,2), (1,5)}
    dict(name="slow_same_string_2_sides", rows=["XXXO", "X.OO", "XOO.", "XO.."], mover=BLACK,
         expect=[("slow_pruned", (2, 2)), ("same_string_twice", (2, 2))]),
    dict(name="capture_2_strings", rows=[".OX", "OX.", "X.."], tail=[(BLACK, (1, 1))], expect_move="multi_capture"),
    dict(name="capture_3_strings", rows=["XO.OX", ".XOX.", "..X.."], tail=[(BLACK, (3, 1))], expect_move="multi_capture"),
    dict(name="capture_4_strings", rows=["..X..", ".XOX.", "XO.OX", ".XOX.", "..X.."], tail=[(BLACK, (3, 3))],
         expect_move="multi_capture"),
    dict(name="capture_21_stones_black", rows=["OOOOOOOX", "OOOOOOOX", "OOOOOOOX", "XXXXXX.."], tail=[(BLACK, (7, 4))],
         expect_move="capture_20"),
    dict(name="capture_21_stones_white", rows=["XXXXXXXO", "XXXXXXXO", "XXXXXXXO", "OOOOOO.."], tail=[(WHITE, (7, 4))],
         expect_move="capture_20"),
    dict(name="merge_3_strings", rows=["X.X", ".X."], tail=[(BLACK, (2, 1))], expect_move="merge_3"),
    dict(name="merge_4_strings", rows=[".O.", "O.O", ".O."], tail=[(WHITE, (2, 2))], expect_move="merge_3"),
    # white to move at (2,1): its own stone (1,1) has that single liberty (the superko quirk's own-colour branch)
    dict(name="own_atari_next_to_candidate", rows=["O..", "X.."], mover=WHITE, expect=[("own_atari_neighbour", (2, 1))]),
    dict(name="eyes_complete", rows=[".XX.XX", "XXXXXX", "......", ".XXX..", ".X.X..", ".XXX.."], mover=BLACK,
         expect=[("complete_eye", (1, 1)), ("complete_eye", (4, 1)), ("complete_eye", (3, 5))]),
    dict(name="eyes_false", rows=[".X.X.X", "XO.OXX", "......", "..OXX.", "..X.X.", "..XXO."], mover=BLACK,
         expect=[("incomplete_eye", (1, 1)), ("incomplete_eye", (5, 1)), ("incomplete_eye", (4, 5))]),
]


def crafted_entry(size: int, spec) -> Entry:
    w = size + 2
    stones = {BLACK: [], WHITE: []}
    for y, row in enumerate(spec["rows"], start=1):
        for x, ch in enumerate(row, start=1):
            if ch in "XO":
                stones[BLACK if ch == "X" else WHITE].append(x + y * w)
    moves = []
    for i in range(max(len(stones[BLACK]), len(stones[WHITE]))):
        for color in (BLACK, WHITE):
            moves.append(stones[color][i] if i < len(stones[color]) else PASS)
    while moves and moves[-1] == PASS:
        moves.pop()
    for color, (x, y) in spec.get("tail", ()):
        if color_after(moves) != color:
            moves.append(PASS)
        moves.append(x + y * w)
    if "mover" in spec and color_after(moves) != spec["mover"]:
        moves.append(PASS)
    entry = Entry(size, tuple(moves), color_after(moves), "crafted:" + spec["name"])
    if "tail" not in spec:                               # the stones stand as drawn (no capture while they were placed)
        board = replay(entry)
        for y, row in enumerate(spec["rows"], start=1):
            for x, ch in enumerate(row, start=1):
                assert board.board[x + y * w] == {"X": BLACK, "O": WHITE, ".": EMPTY}[ch], (spec["name"], x, y)
    return entry


# ---- the corpus ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus(size: int):
    games, plies, step, n_forks, fork_games = PLAN[size]
    entries, forks = [], []
    for g in range(fork_games):
        moves, kos = play_game(size, SEED[size] + g, plies)
        for ply in range(step, plies + 1, step) if g < games else ():
            entries.append(Entry(size, tuple(moves[:ply]), color_after(moves[:ply]), f"game{g}:{ply}"))
        forks += [(g, k, tuple(moves[:k])) for k in kos if k + 2 <= plies]
    # forks spread over the games, earliest first within a game
    forks.sort(key=lambda f: (f[1] // 100, f[0], f[1]))
    forks = forks[:n_forks]
    assert len(forks) == n_forks, (size, len(forks))
    for g, k, rec in forks:
        entries.append(Entry(size, rec, color_after(rec), f"ko:{g}:{k}"))
        entries.append(Entry(size, rec + (PASS, PASS), color_after(rec), f"ko_expired:{g}:{k}"))
    for spec in CRAFTED:
        entries.append(crafted_entry(size, spec))
    short = min(forks, key=lambda f: f[1])[2]               # the shortest fork: its fight ends right below the limit
    for off in HISTORY_OFFSETS:
        target = hmax(size) + off                         # GoBoard.moves at the root = 1 + len(moves)
        pad = target - 3 - len(short)
        assert pad >= 0
        rec = (PASS,) * pad + short + (PASS, PASS)        # an odd pad swaps the colours of the fight, nothing else
        entries.append(Entry(size, rec, color_after(rec), f"history:{off:+d}"))
    assert len(entries) <= LIMITS[size], (size, len(entries))
    return tuple(entries)


def is_history_entry(entry) -> bool:
    return entry.name.startswith("history:")


# ---- the reference-written fixture (tools/gen_golden_rule_corpus.py) --------------------------------------------------------
Fixture = namedtuple("Fixture", "entries cand cells ko_pos ko_move n_moves hash tree_roots")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _unragged(flat, off):
    return [[int(v) for v in flat[off[i]:off[i + 1]]] for i in range(len(off) - 1)]


@functools.lru_cache(maxsize=None)
def load_fixture(size: int) -> Fixture:
    """The corpus as the fixture holds it (no game is replayed to get it) with what the reference found at every entry;
    cand[flag][i] is the candidate list of entry i with check_superko == flag."""
    fix = np.load(os.path.join(GOLDEN, f"rule_corpus_s{size}.npz"))
    moves = _unragged(fix["moves"], fix["moves_off"])
    entries = tuple(Entry(size, tuple(m), int(c), str(n)) for m, c, n in zip(moves, fix["to_move"], fix["names"]))
    cand = tuple(_unragged(fix[f"cand{flag}"], fix[f"cand{flag}_off"]) for flag in (0, 1))
    return Fixture(entries, cand, fix["cells"], fix["ko_pos"], fix["ko_move"], fix["n_moves"], fix["hash"],
                   tuple(int(i) for i in fix["tree_roots"]))


# ---- coverage --------------------------------------------------------------------------------------------------------------
def slow_path_state(board, pos, color):
    """The device's own condition for the exact liberty-union count (gen_candidates): None if the fast path decides, else
    (kept, number of distinct friendly strings, a string seen on two sides)."""
    if board.n_empty_neighbors(pos) > 1:
        return None
    other = opponent(color)
    ids = []
    twice = False
    for n in board.neighbor4(pos):
        c = board.board[n]
        if c == color:
            if board.num_liberties(n) >= 3:
                return None
            if board.sid[n] in ids:
                twice = True
            else:
                ids.append(board.sid[n])
        elif c == other and board.num_liberties(n) == 1:
            return None
    size = sum(len(board.strings[k].stones) for k in ids)
    if size + 1 < 7:
        return None
    return board.check_self_atari_stone(pos, color) == 0, len(ids), twice


def point_categories(board, pos, color):
    """Categories of the empty point `pos` for `color` to move on a superko-checking oracle board."""
    out = []
    if board.board[pos] != EMPTY:
        return out
    if board.n_empty_neighbors(pos) == 0 and board._is_suicide(pos, color):
        return ["suicide"]
    if board.ko_pos == pos and board.ko_move == board.moves - 1:
        return ["ko"]
    if any(board.board[n] == color and board.num_liberties(n) == 1 for n in board.neighbor4(pos)):
        out.append("own_atari_neighbour")
    if not board.is_legal(pos, color):
        return out + ["superko_only"]
    if board.is_complete_eye(pos, color):
        return out + ["complete_eye"]
    if board.eye_color(pos) == color:
        out.append("incomplete_eye")
    slow = slow_path_state(board, pos, color)
    if slow is not None:
        kept, n_strings, twice = slow
        out += ["slow_entered", "slow_kept" if kept else "slow_pruned"]
        if n_strings >= 2:
            out.append("slow_multi")
        if twice:
            out.append("same_string_twice")
    return out


def move_categories(board, pos, color):
    """Categories of the move `pos` about to be played on `board` (before put_stone)."""
    if pos == PASS:
        return []
    other = opponent(color)
    dead, friends = set(), set()
    for n in board.neighbor4(pos):
        if board.board[n] == other and board.strings[board.sid[n]].libs == {pos}:
            dead.add(board.sid[n])
        elif board.board[n] == color:
            friends.add(board.sid[n])
    out = []
    stones = sum(len(board.strings[k].stones) for k in dead)
    if dead:
        out.append("capture")
    if len(dead) >= 2:
        out.append("multi_capture")
    if stones >= 20:
        out.append("capture_20")
    if len(friends) >= 3:
        out.append("merge_3")
    if not friends and stones == 1 and board.n_empty_neighbors(pos) == 0:
        out.append("ko_set")
    return out


def position_counts(board, color) -> Counter:
    counts = Counter()
    for pos in board.onboard_pos:
        counts.update(point_categories(board, pos, color))
    return counts


def coverage(entries) -> Counter:
    """Position/point pairs per point category over the entries' positions, and moves per move category over the distinct
    record prefixes (a move shared by two samples of one game counts once)."""
    counts = Counter()
    seen = set()
    for entry in entries:
        board = GoBoard(entry.size, 7.0, True)
        color, key = BLACK, 0
        for pos in entry.moves:
            key = hash((key, pos))
            if key not in seen:
                seen.add(key)
                counts.update(move_categories(board, pos, color))
            board.put_stone(pos, color)
            color = opponent(color)
        counts.update(position_counts(board, color))
    return counts


# ---- roots of the short searches ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tree_roots(size: int):
    """Indices of the corpus entries the short searches start from: dense positions where the side to move can take a ko,
    capture, or faces slow-path points, with few enough candidates that 41 descents reach most root children."""
    scored = []
    entries = corpus(size)
    for index, entry in enumerate(entries):
        if is_history_entry(entry) or entry.name.startswith("crafted:") or len(entry.moves) + 8 >= hmax(size):
            continue
        board = replay(entry)
        color = entry.to_move
        cands = board.search_candidates(color)
        kinds = Counter()
        for pos in cands[:-1]:
            kinds.update(move_categories(board, pos, color))
        here = position_counts(board, color)
        score = 6 * min(kinds["ko_set"], 2) + min(kinds["capture"], 6) + 3 * min(here["slow_entered"], 2) \
            + (4 if len(cands) <= 40 else 0) + (2 if entry.name.startswith("ko") else 0)
        scored.append((-score, index))
    scored.sort()
    chosen, records = [], set()
    for _, index in scored:                              # (a ko fork may coincide with a sampled ply of its game)
        if entries[index].moves not in records and len(chosen) < N_TREE_ROOTS[size]:
            records.add(entries[index].moves)
            chosen.append(index)
    return tuple(sorted(chosen))


# ---- comparison code of the GPU tests ------------------------------------------------------------------------------------------
class CorpusMismatch(AssertionError):
    pass


def check_roots(entries, expected, got):
    """`got`: the root action list of every tree (lists of ints, in any iterable), `expected`: the fixture's lists."""
    if hasattr(got, "__len__") and len(got) != len(entries):
        raise CorpusMismatch(f"{len(got)} trees for {len(entries)} entries")
    count = 0
    for index, (entry, want, have) in enumerate(zip(entries, expected, got)):
        if [int(v) for v in have] != [int(v) for v in want]:
            raise CorpusMismatch(f"entry {index} ({entry.name}): root candidates differ\n want {list(want)}\n got  {list(have)}")
        count += 1
    if count != len(entries):
        raise CorpusMismatch(f"{count} trees for {len(entries)} entries")


def walk_tree(entry, nodes, superko: bool = True):
    """Walk a tree from its root through children_index, replay every node's path on the oracle board and compare the node's
    action list with search_candidates there.  `nodes[i]` = (action list, children_index list).  Returns, per node index,
    (board, colour to move, categories of the move that led there)."""
    root = replay(entry, superko)
    reached = {0: (root, entry.to_move, [])}
    order = [0]
    while order:
        index = order.pop()
        board, color, _ = reached[index]
        action, children = nodes[index]
        want = board.search_candidates(color)
        if [int(a) for a in action] != want:
            raise CorpusMismatch(f"{entry.name}: node {index} at move {board.moves}: candidates differ\n want {want}\n"
                                 f" got  {[int(a) for a in action]}")
        if len(children) != len(action):
            raise CorpusMismatch(f"{entry.name}: node {index}: {len(children)} child links for {len(action)} actions")
        for move, child in zip(action, children):
            child = int(child)
            if child < 0:
                continue
            if child in reached or not 0 < child < len(nodes):
                raise CorpusMismatch(f"{entry.name}: node {index}: child link {child} is not a fresh node of the tree")
            kinds = move_categories(board, int(move), color)
            nxt = board.clone()
            nxt.put_stone(int(move), color)
            reached[child] = (nxt, opponent(color), kinds)
            order.append(child)
    if len(reached) != len(nodes):
        raise CorpusMismatch(f"{entry.name}: {len(nodes)} nodes, {len(reached)} reachable from the root")
    return reached


def check_leaves(entry, reached, leaves):
    """`leaves`: (node index, planes [6][S][S]) of every evaluated leaf; the planes are those of the node's position."""
    from oracle.feature import generate_input_planes
    for node, planes in leaves:
        board, color, _ = reached[int(node)]
        want = generate_input_planes(board, color)
        if not np.array_equal(np.asarray(planes, dtype=np.float32), want):
            raise CorpusMismatch(f"{entry.name}: planes of the leaf at node {node} differ")


def expanded_coverage(reached_per_tree) -> Counter:
    """What the expanded NON-ROOT nodes hold: nodes with a ko-forbidden point, with a slow-path point, after a capture."""
    counts = Counter()
    for reached in reached_per_tree:
        for index, (board, color, kinds) in reached.items():
            if index == 0:
                continue
            here = position_counts(board, color)
            counts["nodes"] += 1
            counts["ko_node"] += here["ko"] > 0
            counts["superko_node"] += here["superko_only"] > 0
            counts["slow_node"] += here["slow_entered"] > 0
            counts["after_capture"] += "capture" in kinds
            counts["after_ko_set"] += "ko_set" in kinds
    return counts


EXPANDED_MINIMUMS = {9: {"ko_node": 3, "after_capture": 10, "slow_node": 2}, 13: {"ko_node": 3},
                     19: {"ko_node": 3, "after_capture": 10, "slow_node": 2}}


# ---- a stand-in for the device, and the ways it may be wrong ---------------------------------------------------------------------
class _NoSuperko(GoBoard):
    def is_legal(self, pos, color):
        keep, self.check_superko = self.check_superko, False
        try:
            return GoBoard.is_legal(self, pos, color)
        finally:
            self.check_superko = keep


class _NoKo(GoBoard):
    def is_legal(self, pos, color):
        keep, self.ko_pos = self.ko_pos, -1
        try:
            return GoBoard.is_legal(self, pos, color)
        finally:
            self.ko_pos = keep


class _Threshold8(GoBoard):
    def search_candidates(self, color):
        out = [p for p in self.get_all_legal_pos(color)
               if self.check_self_atari_stone(p, color) < 8 and not self.is_complete_eye(p, color)]
        return out + [PASS]


class _EdgeEye3(GoBoard):
    def is_complete_eye(self, pos, color):
        if self.eye_color(pos) != color:
            return False
        count = 0
        for c in self.cross4(pos):
            v = self.board[c]
            if v == color or v == OUT_OF_BOARD or (v == EMPTY and self.eye_color(c) == color):
                count += 1
        return count >= 3


class _NoDedup(GoBoard):
    """Liberties of a string that touches the point on two sides are counted once per side."""
    def check_self_atari_stone(self, pos, color):
        libs = set((n, 0) for n in self.neighbor4(pos) if self.board[n] == EMPTY)
        if len(libs) > 1:
            return 0
        other = opponent(color)
        seen = {}
        size = 0
        for n in self.neighbor4(pos):
            c = self.board[n]
            if c == color:
                k = self.sid[n]
                tag = seen.get(k, 0)
                libs |= set((p, tag) for p in self.strings[k].libs)
                if len(libs) >= 3:
                    return 0
                if tag == 0:
                    size += len(self.strings[k].stones)
                seen[k] = tag + 1
            elif c == other and self.num_liberties(n) == 1:
                return 0
        return size + 1


PERTURBATIONS = {"self_atari_threshold_8": _Threshold8, "superko_ignored": _NoSuperko, "ko_ignored": _NoKo,
                 "edge_eye_count_3": _EdgeEye3, "liberty_union_not_deduplicated": _NoDedup}

def _keeps_class(cls):
    """GoBoard.clone builds a plain GoBoard: keep the class, so that a perturbed rule holds below the root too."""
    def clone(self):
        b = cls(self.board_size, self.komi, self.check_superko)
        b.copy_from(self)
        return b
    cls.clone = clone


for _cls in PERTURBATIONS.values():
    _keeps_class(_cls)


class OracleReader:
    """The reader interface of the comparison code on top of oracle.tree.MCTSTree + StubNet: root action lists of all trees,
    the nodes of a tree as (action list, children_index), the leaf planes with their node indices."""

    def __init__(self, entries, superko: bool = True, board_cls=GoBoard, salt: int = 3, batch: int = 16):
        self.entries = entries
        self.superko = superko
        self.board_cls = board_cls
        self.salt = salt
        self.batch = batch
        self.trees = {}

    def root_actions(self):
        for entry in self.entries:
            board = replay(entry, self.superko, self.board_cls)
            yield board.search_candidates(entry.to_move)

    def search(self, tree: int, batches=(16, 16, 9)):
        from oracle.stubnet import StubNet
        from oracle.tree import MCTSTree
        entry = self.entries[tree]
        board = replay(entry, self.superko, self.board_cls)
        np.random.seed(100 + tree)
        mcts = MCTSTree(StubNet(self.salt), entry.size, tree_size=64, batch_size=self.batch)
        leaves = []

        def hook(planes, _policy, _value, _logit, mcts=mcts):
            leaves.extend(zip(list(mcts.batch_queue.node_index), planes.numpy().copy()))

        mcts.eval_hook = hook
        mcts._initialize_search(board, entry.to_move)
        work = board.clone()
        for leaves_in_batch in batches:
            for _ in range(leaves_in_batch):
                work.copy_from(board)
                mcts.search_mcts(work, entry.to_move, mcts.current_root, [])
            if mcts.batch_queue.node_index:
                mcts.process_mini_batch(board)
        self.trees[tree] = (mcts, leaves)

    def nodes(self, tree: int):
        mcts, _ = self.trees[tree]
        return [(list(n.action[:n.num_children]), [int(c) for c in n.children_index[:n.num_children]])
                for n in mcts.node[:mcts.num_nodes]]

    def leaves(self, tree: int):
        return self.trees[tree][1]
