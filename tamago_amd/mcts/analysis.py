"""Batch analysis: every position searched as its own PUCT tree, many trees in lock-step on one SearchEngine.

No reference counterpart: the reference analyses one position at a time (gtp/client.py lz-analyze / cgos-analyze over
mcts/tree.py).  The equivalence contract: position k analysed with seed s_k gives what

    np.random.seed(s_k)
    tree = MCTSTree(network, tree_size=visits + 16, batch_size=batch_size, cgos_mode=cgos_mode)
    best = tree.search_best_move(board_k, color_k, TimeManager(TimeControl.STRICT_PLAYOUT, visits), {})
    tree.get_root().get_analysis(board_k, "lz" | "cgos", tree.get_pv_lists)

gives, byte for byte, whatever the number of trees per engine (max_trees); with mode=TimeControl.CONSTANT_PLAYOUT the
TimeManager of the contract is TimeManager(TimeControl.CONSTANT_PLAYOUT, visits) - the reference's default search, which
stops once the runner-up child cannot catch up: the test runs on the device behind each full mini-batch and halts the
trees it decides while the others go on (SearchEngine.puct_chain(early_total=visits)):
- every tree draws from its own stream, np.random.RandomState(s_k).get_state();
- the mini-batches are those of MCTSTree.search's STRICT_PLAYOUT path: the root evaluation, then `visits` descents in
  mini-batches of batch_size, the last one partial (chained with puct_chain where the engine allows it);
- a root whose only candidate is PASS answers PASS without a search (its analysis is that of the evaluated root), a best
  child valued below RESIGN_THRESHOLD answers RESIGN (mcts/tree.py:57-105);
- the analysis strings come from MCTSNode.get_analysis_status_list / get_analysis_from_status_list over one
  tg_search_read_analysis read-out (root statistics and principal variations of all trees in one launch).
"""
import copy
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from tamago_amd.board.constant import PASS, RESIGN
from tamago_amd.board.go_board import GoBoard
from tamago_amd.board.stone import Stone, color_value
from tamago_amd.mcts.constant import RESIGN_THRESHOLD
from tamago_amd.mcts.engine import SearchEngine, evaluator_for
from tamago_amd.mcts.node import MCTSNode
from tamago_amd.mcts.time_manager import TimeControl

# Device memory the node pools of one engine may take by default (max_trees).  A pool node holds A children x (3 int32 +
# 3 float64 + 1 int16) plus its 32-byte record: 3 148 bytes at 9x9, 13 788 at 19x19.
POOL_BUDGET_BYTES = 8 << 30
MAX_TREES = 2048


def pool_bytes_per_node(board_size: int) -> int:
    a = board_size * board_size + 1
    return a * (3 * 4 + 3 * 8 + 2) + 32


def tree_size_for(visits: int) -> int:
    """Nodes per tree: every descent creates at most one node (bench.py sizes its pools the same way)."""
    return visits + 16


def default_max_trees(board_size: int, visits: int, budget: int = POOL_BUDGET_BYTES) -> int:
    per_tree = tree_size_for(visits) * pool_bytes_per_node(board_size)
    return max(1, min(MAX_TREES, budget // per_tree))


def plan_chunks(count: int, max_trees: int) -> Tuple[int, List[Tuple[int, int]]]:
    """(trees per engine, [(first, end), ...]): the fewest chunks of at most max_trees positions, as even as possible; the
    engine has as many trees as the largest chunk (a shorter last chunk fills its spare trees with copies of its last
    position, whose results are dropped)."""
    if count <= 0:
        return 0, []
    if max_trees < 1:
        raise ValueError(f"max_trees {max_trees} < 1")
    chunks = -(-count // max_trees)
    trees = -(-count // chunks)
    return trees, [(lo, min(lo + trees, count)) for lo in range(0, count, trees)]


def game_seeds(seed: int, count: int) -> List[int]:
    """Seed of position k of one game: seed + k (a game's output does not depend on the other games analysed with it)."""
    return [seed + k for k in range(count)]


@dataclass
class PositionAnalysis:
    """The analysis of one position.  best_move: padded coordinate (PASS 0, RESIGN -1); visits / value_sum: the root's
    node_visits and node_value_sum (float32); status: MCTSNode.get_analysis_status_list's list (visited children,
    most visited first, with their PVs)."""
    best_move: int
    visits: int
    value_sum: float
    status: List[dict]
    board_size: int = 9

    @property
    def winrate(self) -> Optional[float]:
        """The root winrate of the cgos line (None for a root without visits)."""
        return float(self.value_sum) / self.visits if self.visits else None

    def _root(self) -> MCTSNode:
        root = MCTSNode(0)
        root.node_visits = self.visits
        root.node_value_sum = np.float32(self.value_sum)
        return root

    def lz(self) -> str:
        """The lz-analyze info line (ends with a newline)."""
        return self._root().get_analysis_from_status_list("lz", self.status)

    def cgos(self) -> str:
        """The cgos-analyze JSON line (ends with a newline); a root without visits has none (ZeroDivisionError, like the
        single-tree path)."""
        return self._root().get_analysis_from_status_list("cgos", self.status)

    def best_move_gtp(self) -> str:
        from tamago_amd.board.coordinate import Coordinate
        return Coordinate(self.board_size).convert_to_gtp_format(self.best_move)

    def move_stats(self, move: str):
        """(visits, winrate, rank) of the root child played as `move` (GTP text); (0, None, None) if it was not visited."""
        for st in self.status:
            if st["move"] == move:
                return st["visits"], st["winrate"], st["order"]
        return 0, None, None


def _best_move(root: MCTSNode) -> int:
    index = root.get_best_move_index()
    if root.calculate_value_evaluation(index) < RESIGN_THRESHOLD:
        return RESIGN
    return root.action[index]


class CachedAnalyses(list):
    """What analyze_positions(eval_cache=entries) returns: the analyses, and what the cache did (cache_report)."""
    cache_report: Optional[dict] = None


def analyze_positions(network, positions: Sequence[Tuple[GoBoard, object]], visits: int, batch_size: int = 16,
                      max_trees: Optional[int] = None, cgos_mode: bool = False, check_superko: bool = False,
                      seeds: Optional[Sequence[int]] = None, pv_depth: int = 32,
                      device_index: int = 0, records=None, board_size: Optional[int] = None,
                      mode: TimeControl = TimeControl.STRICT_PLAYOUT, compact_idle: bool = False,
                      eval_cache: Optional[int] = None) -> List[PositionAnalysis]:
    """Analyse (board, colour to move) pairs of one board size, one tree per position (see the module docstring for the
    contract).  seeds default to 0, 1, 2, ...; max_trees defaults to default_max_trees.  check_superko must match the
    boards' own setting (as MCTSTree takes it from the board).
    records: positions are (record index, ply) members of these game records (mcts/record_roots.py) on boards of
    board_size, and the roots are written on the device from the records (SearchEngine.set_roots_from_records) - no board
    is replayed or copied on the host; same output.
    mode: STRICT_PLAYOUT (every position gets `visits` descents) or CONSTANT_PLAYOUT (each tree stops early by the
    reference's rule, on the device).
    compact_idle: trees that do not search are left out of the forward passes - in CONSTANT_PLAYOUT mode the
    halted ones (pass-only roots, decided positions, as of the search's last look), in STRICT_PLAYOUT mode the trees of a last,
    partial chunk that repeat its last position, which are halted for it.  Same output.
    eval_cache (entries, None / 0: off): an evaluation cache of that many entries serves the positions whose
    outputs it holds - the plies of one record searched side by side overlap - for the whole call; the searches go
    mini-batch by mini-batch then.  Same output; the list returned is then a CachedAnalyses, whose cache_report holds
    forward_positions (handed over), evaluated_positions and eval_cache_stats."""
    from tamago_amd.mcts.reanalyse import set_chunk_roots
    if mode not in (TimeControl.STRICT_PLAYOUT, TimeControl.CONSTANT_PLAYOUT):
        raise ValueError("analyze_positions: mode must be STRICT_PLAYOUT or CONSTANT_PLAYOUT")
    early_stop = mode == TimeControl.CONSTANT_PLAYOUT
    positions = list(positions)
    if not positions:
        return []
    if records is not None:
        from tamago_amd.mcts.record_roots import pack_record_roots
        if board_size is None:
            raise ValueError("analyze_positions: records need board_size")
        size = board_size
        pack_record_roots(records, positions)             # (bad input raises here, before an engine exists)
    else:
        size = positions[0][0].board_size
    if records is None and any(board.board_size != size for board, _ in positions):
        raise ValueError("analyze_positions: positions of several board sizes")
    net_size = getattr(network, "board_size", None)
    if net_size is not None and net_size != size:
        raise ValueError(f"network is built for {net_size}x{net_size}, boards are {size}x{size}")
    if visits < 1 or batch_size < 1:
        raise ValueError("analyze_positions: visits and batch_size must be at least 1")
    seeds = list(range(len(positions))) if seeds is None else [int(s) for s in seeds]
    if len(seeds) != len(positions):
        raise ValueError("analyze_positions: one seed per position")
    trees, chunks = plan_chunks(len(positions), max_trees or default_max_trees(size, visits))
    cache = None
    if eval_cache:
        from tamago_amd.nn.eval_cache import EvalCache
        cache = EvalCache(size, int(eval_cache), device_index=device_index)
    engine = SearchEngine(size, trees, tree_size_for(visits), batch_size, evaluator_for(network, device_index, cache),
                          cgos_mode, check_superko, device_index)
    batches = [batch_size] * (visits // batch_size) + ([visits % batch_size] if visits % batch_size else [])
    results: List[PositionAnalysis] = []
    coordinates = BoardCoordinates(size)
    try:
        for lo, hi in chunks:
            members = [lo + min(k, hi - lo - 1) for k in range(trees)]
            set_chunk_roots(engine, positions, members, seeds, records, check_superko)
            engine.root_eval(use_logit=False)
            pass_only = np.asarray(engine.root_children) == 1          # tree.py:76-77: PASS without a search
            early = engine.read_analysis(pv_depth) if pass_only[:hi - lo].any() else None
            if early_stop and pass_only.any():
                engine.set_halt(pass_only)                             # (answered already: no search, no draws)
            if early_stop:
                engine.puct_chain(batches, early_total=visits, compact=compact_idle)
            elif compact_idle:
                spare = np.arange(trees) >= hi - lo                    # (filled with the chunk's last position: nobody reads them)
                if spare.any():
                    engine.set_halt(spare)
                engine.puct_chain(batches, compact=True)
            elif engine.can_chain(visits):
                engine.puct_chain(batches)
            else:
                for leaves in batches:
                    engine.ensure_capacity(leaves)
                    engine.puct_batch(leaves)
            final = engine.read_analysis(pv_depth)
            for k in range(hi - lo):
                root, pv_lists = (early if pass_only[k] else final)[k]
                board = positions[lo + k][0] if records is None else coordinates
                status = root.get_analysis_status_list(board, pv_lists)
                best = PASS if pass_only[k] else _best_move(root)
                results.append(PositionAnalysis(best, root.node_visits, float(root.node_value_sum), status, size))
        if cache is not None:
            results = CachedAnalyses(results)
            results.cache_report = dict(forward_positions=engine.forward_positions, evaluated_positions=sum(engine.evaluator.batches),
                                        eval_cache_stats=dict(cache.stats(), entries=cache.entries, caches=1))
    finally:
        engine.close()
        if cache is not None:
            cache.close()
    return results


# ---- game records -----------------------------------------------------------------------------------------------------
@dataclass
class GamePosition:
    """Position `move_number - 1` of a game record: the board before move `move_number` (1-based), or the final position
    (played None).  color: the side to move (the colour of the move played there; after the last move, its opponent)."""
    game: str
    move_number: int
    color: Stone
    played: Optional[int]
    board: GoBoard = field(repr=False)


def game_positions(sgf, superko: bool = False, name: str = "") -> List[GamePosition]:
    """Every position of a record (an SGFReader) replayed like GTP loadsgf: a fresh board of the record's SZ and KM, the
    moves in order.  One position before each move and the final one."""
    size = sgf.board_size
    if size not in (9, 13, 19):
        raise ValueError(f"{name or 'record'}: board size {size} is not supported (9, 13 or 19)")
    board = GoBoard(board_size=size, komi=sgf.komi, check_superko=superko)
    out = []
    n = sgf.get_n_moves()
    for i in range(n + 1):
        if i < n:
            color = sgf.get_color(i)
            played = sgf.get_move_data(i)
        else:
            color = board.get_to_move()
            played = None
        out.append(GamePosition(name, i + 1, color, played, copy.deepcopy(board)))
        if i < n:
            board.put_stone(played, color)
    return out


class BoardCoordinates:
    """What the output code reads of a position's board (MCTSNode.get_analysis_status_list, GameAnalysis.played_gtp,
    annotated_sgf): its size and its Coordinate.  Stands in for the replayed board of a position whose root is written on
    the device."""

    def __init__(self, board_size: int):
        from tamago_amd.board.coordinate import Coordinate
        self.board_size = board_size
        self.coordinate = Coordinate(board_size)


def game_record_positions(sgf, name: str = ""):
    """game_positions without a board: ((moves, colours), [GamePosition]) - the record with the SGF's own colour tags, as
    SearchEngine.set_roots_from_records takes it, and the same positions (position k is ply k of the record) with a
    BoardCoordinates in place of the replayed board.  Nothing is replayed or copied."""
    from tamago_amd.mcts.record_roots import to_move_at
    size = sgf.board_size
    if size not in (9, 13, 19):
        raise ValueError(f"{name or 'record'}: board size {size} is not supported (9, 13 or 19)")
    n = sgf.get_n_moves()
    moves = [int(sgf.get_move_data(i)) for i in range(n)]
    colors = [sgf.get_color(i) for i in range(n)]
    board = BoardCoordinates(size)
    out = [GamePosition(name, i + 1, colors[i], moves[i], board) for i in range(n)]
    out.append(GamePosition(name, n + 1, Stone(to_move_at(colors, n, n)), None, board))
    return (moves, colors), out


@dataclass
class GameAnalysis:
    position: GamePosition
    analysis: PositionAnalysis

    def played_gtp(self) -> Optional[str]:
        if self.position.played is None:
            return None
        return self.position.board.coordinate.convert_to_gtp_format(self.position.played)

    def record(self) -> dict:
        """The JSONL record of the position."""
        a = self.analysis
        played = self.played_gtp()
        pv, pw, pr = a.move_stats(played) if played is not None else (None, None, None)
        return {"game": self.position.game, "move_number": self.position.move_number,
                "color": "B" if color_value(self.position.color) == 1 else "W",
                "best": a.best_move_gtp(), "visits": a.visits, "winrate": a.winrate,
                "played": played, "played_visits": pv, "played_winrate": pw, "played_rank": pr,
                "moves": a.status}

    def comment(self) -> str:
        """SGF comment of the move played in this position (see tamago_amd/analyze.py)."""
        a = self.analysis
        side = "B" if color_value(self.position.color) == 1 else "W"
        best = a.best_move_gtp()
        best_visits = next((st["visits"] for st in a.status if st["move"] == best), 0)
        text = f"{side} to move, winrate {_pct(a.winrate)}, best {best} ({best_visits} visits)"
        played = self.played_gtp()
        if played is not None:
            pv, pw, _ = a.move_stats(played)
            text += f", played {played} ({pv} visits, winrate {_pct(pw)})"
        top = ", ".join(f"{st['move']} {st['visits']} {_pct(st['winrate'])}" for st in a.status[:3])
        return text + f", top: {top or '-'}"


def _pct(value: Optional[float]) -> str:
    return "-" if value is None or math.isnan(value) else f"{100.0 * value:.1f}%"


def analyze_game(network, sgf_path: str, visits: int, seed: int = 0, superko: bool = False, device_roots: bool = False,
                 **kwargs) -> List[GameAnalysis]:
    """Analyse every position of one game record (game_positions) with seeds seed + k; kwargs go to analyze_positions.
    device_roots: the positions, the final one included, are set up on the device from the record with the SGF's own
    colour tags (game_record_positions) - no position is replayed or copied on the host; same output."""
    from tamago_amd.sgf.reader import SGFReader
    if device_roots:
        sgf = SGFReader(sgf_path, 9)
        record, positions = game_record_positions(sgf, sgf_path)
        results = analyze_positions(network, [(0, k) for k in range(len(positions))], visits, check_superko=superko,
                                    seeds=game_seeds(seed, len(positions)), records=[record], board_size=sgf.board_size,
                                    **kwargs)
        return [GameAnalysis(p, a) for p, a in zip(positions, results)]
    positions = game_positions(SGFReader(sgf_path, 9), superko, sgf_path)
    results = analyze_positions(network, [(p.board, p.color) for p in positions], visits, check_superko=superko,
                                seeds=game_seeds(seed, len(positions)), **kwargs)
    return [GameAnalysis(p, a) for p, a in zip(positions, results)]


def annotated_sgf(analyses: Sequence[GameAnalysis], sgf) -> str:
    """The record's moves with the comment of each move (GameAnalysis.comment of the position it was played in)."""
    size = sgf.board_size
    head = f"(;FF[4]GM[1]SZ[{size}]KM[{sgf.komi}]"
    if sgf.black_player_name:
        head += f"PB[{sgf.black_player_name}]"
    if sgf.white_player_name:
        head += f"PW[{sgf.white_player_name}]"
    parts = [head]
    for g in analyses:
        if g.position.played is None:
            continue
        color = "B" if color_value(g.position.color) == 1 else "W"
        pos = g.position.played
        coord = "" if pos == PASS else g.position.board.coordinate.convert_to_sgf_format(pos)
        parts.append(f";{color}[{coord}]C[{g.comment().replace(']', ')')}]")
    return "".join(parts) + ")\n"
