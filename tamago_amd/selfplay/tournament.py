"""Round-robin tournaments between networks under PUCT search: every game of every pairing in ONE lock-step engine.

    python -m tamago_amd.tournament --models a.bin b.bin c.bin [--names A B C] --visits V --batch-size K
                                    [--games-per-pair R] [--boards N] [--size S] [--komi 7.0] [--seed-base 0] [--save-dir DIR]

A game is the puct_match game (selfplay/puct_match.py) of its black network, its white network and its seed, both
setups (visits, batch_size) and strict - byte for byte, whatever else shares the launch and however many slots the engine has.
The schedule (`schedule`): for round r in range(games_per_pair), for every ordered pair (i, j), i != j, in lexicographic order,
one game with entrant i as black and j as white; game n - the running number - draws from the legacy stream seeded with
(seed_base + n) % 2**32.

What puct_match cannot do, and this driver does: a call moves EVERY live game by one ply, whatever its colour
and whichever network has to move.  A tree's group is the entrant index of the side to move in its game; the grouped ranks
(SearchEngine.group_live) sort the live trees by group, so that one compact selection serves the trees of every network, each
network's forward pass runs over one contiguous segment of the plane rows, and one compact backup finishes the mini-batch.  A
freed slot takes the next game of the schedule before the very next call - there is no parity rule and nothing parks - and
slots without a game are halted: rank -1, no descent, no row.  A call is

    1. SearchEngine.root_eval_groups: root planes, the slots without a game halted, grouped ranks, a gather of the planes to
       rows by rank, one evaluator call per group that has live trees, a scatter back, the strided root backup
    2. tg_search_best_moves(play = 0): which roots have one child
    3. SearchEngine.puct_chain_groups: the mini-batches, by the same ranks (one-child roots search on, as in a strict
       puct_match call: their streams are put back around the launches)
    4. tg_search_best_moves(play = 1): the move of every live game, decided and played on the device
    5. the host's bookkeeping: move lists, passes, the ends of games, count_score of the boards two passes ended, new games

Ratings: a Bradley-Terry maximum-likelihood fit on the pooled pair results (`bradley_terry_elo`).
"""
import argparse
import json
import math
import os
import time
from typing import List, Optional, Sequence

import numpy as np

from tamago_amd.board.constant import PASS, RESIGN
from tamago_amd.board.stone import Stone
from tamago_amd.mcts.constant import RESIGN_THRESHOLD
from tamago_amd.selfplay.puct_match import EngineSetup, _Game, game_result, mini_batches, record_text

MAX_ENTRANTS = 64                                  # the groups of one launch (tg_search_group_live)


def schedule(n_entrants: int, games_per_pair: int = 1):
    """[(black, white), ...] by game index: for every round, every ordered pair of distinct entrants in lexicographic order."""
    if n_entrants < 2:
        raise ValueError("schedule: at least two entrants")
    if games_per_pair < 1:
        raise ValueError("schedule: games_per_pair must be >= 1")
    return [(i, j) for _ in range(games_per_pair) for i in range(n_entrants) for j in range(n_entrants) if i != j]


def game_seed(seed_base: int, index: int) -> int:
    return (int(seed_base) + int(index)) % 2 ** 32


def pooled_wins(crosstable) -> np.ndarray:
    """w[i][j]: what i scored against j over both colours - a win 1, a draw half a win for each side; unfinished games none."""
    n = len(crosstable)
    w = np.zeros((n, n), dtype=np.float64)
    for i in range(n):
        for j in range(n):
            cell = crosstable[i][j]
            if i == j or cell is None:
                continue
            w[i, j] += cell["wins"] + 0.5 * cell["draws"]                 # i as black
            w[j, i] += cell["losses"] + 0.5 * cell["draws"]
    return w


def bradley_terry_elo(wins, tolerance: float = 1e-14, max_iterations: int = 1000000) -> List[Optional[float]]:
    """Bradley-Terry maximum-likelihood ratings in Elo units from wins[i][j] (i's score against j, fractional counts allowed):
    P(i beats j) = p_i / (p_i + p_j), elo_i = 400 log10 p_i, shifted so that the rated entrants' mean is 0.  The MM iteration
    p_i <- W_i / sum_j n_ij / (p_i + p_j) in float64 to a fixed point.  An entrant that won or lost all of its decided games
    (or has none) has no finite rating: None, and it is left out of the fit - repeatedly, since leaving one out can leave
    another without a loss or a win among the rest.  For two entrants the difference is 400 log10(w_01 / w_10), match.rating's
    elo."""
    w = np.array(wins, dtype=np.float64)
    n = len(w)
    assert w.shape == (n, n)
    np.fill_diagonal(w, 0.0)
    rated = np.ones(n, dtype=bool)
    while True:
        sub = w * np.outer(rated, rated)
        won, lost = sub.sum(axis=1), sub.sum(axis=0)
        keep = rated & (won > 0) & (lost > 0)
        if (keep == rated).all():
            break
        rated = keep
    out: List[Optional[float]] = [None] * n
    idx = np.flatnonzero(rated)
    if len(idx) < 2:
        return out
    sub = w[np.ix_(idx, idx)]
    games = sub + sub.T
    won = sub.sum(axis=1)
    p = np.ones(len(idx), dtype=np.float64)
    for _ in range(max_iterations):
        denom = (games / (p[:, None] + p[None, :])).sum(axis=1)
        new = won / denom
        new /= np.exp(np.mean(np.log(new)))
        done = np.max(np.abs(np.log(new) - np.log(p))) < tolerance
        p = new
        if done:
            break
    elo = 400.0 * np.log10(p)
    elo -= elo.mean()
    for k, i in enumerate(idx):
        out[int(i)] = float(elo[k])
    return out


def _check_entrants(entrants, size):
    entrants = list(entrants)
    if not 2 <= len(entrants) <= MAX_ENTRANTS:
        raise ValueError(f"puct_tournament: {len(entrants)} entrants (2 to {MAX_ENTRANTS})")
    names = []
    for entry in entrants:
        if isinstance(entry, EngineSetup):
            raise ValueError("puct_tournament: an entrant is (name, network); visits or mini-batches per entrant are not built - "
                             "one `visits` and one `batch_size` hold for everybody")
        if not isinstance(entry, (tuple, list)) or len(entry) != 2 or not isinstance(entry[0], str):
            raise ValueError("puct_tournament: an entrant is (name, network)")
        net_size = getattr(entry[1], "board_size", None)
        if net_size is not None and net_size != size:
            raise ValueError(f"puct_tournament: {entry[0]}: network is built for {net_size}x{net_size}, the tournament is {size}x{size}")
        names.append(entry[0])
    if len(set(names)) != len(names):
        raise ValueError("puct_tournament: the entrants' names must be distinct")
    return names, [entry[1] for entry in entrants]


class _Table:
    """One lock-step engine of `boards` slots and the games on it."""

    def __init__(self, names, networks, visits, batch_size, size, komi, boards, cgos_mode, check_superko, resign_threshold, save_dir,
                 device_index, make_engine):
        from tamago_amd.board.go_board import GoBoard
        self.names, self.networks = names, networks
        self.visits, self.batch_size = visits, batch_size
        self.size, self.boards, self.threshold, self.save_dir = size, boards, float(resign_threshold), save_dir
        self.start_board = GoBoard(board_size=size, komi=komi, check_superko=check_superko)
        self.komi = float(self.start_board.get_komi())
        self.max_moves = 2 * size * size
        if make_engine is None:
            from tamago_amd.mcts.engine import SearchEngine, evaluator_for
            self.evaluators = [evaluator_for(net, device_index) for net in networks]
            self.engine = SearchEngine(size, boards, visits + 16, batch_size, self.evaluators[0], cgos_mode, check_superko, device_index)
        else:
            self.evaluators = list(networks)
            self.engine = make_engine(self)
        self.slots = [None] * boards                        # the _Game in progress

    def close(self):
        self.engine.close()

    def _mover(self, game) -> int:
        """The entrant to move: black on even plies (a resignation ends the game, every other move is recorded)."""
        return game.black if len(game.moves) % 2 == 0 else game.white

    def play(self, queue, stats, on_finished):
        engine = self.engine
        queue = list(queue)
        batches = mini_batches(self.visits, self.batch_size)
        while queue or any(g is not None for g in self.slots):
            for slot in range(self.boards):
                if self.slots[slot] is None and queue:
                    game = queue.pop(0)
                    self.slots[slot] = game
                    engine.set_root(slot, self.start_board, Stone.BLACK, np.random.RandomState(game.seed).get_state())
                    if stats["calls"]:
                        stats["restarts"] += 1
            live = [slot for slot, g in enumerate(self.slots) if g is not None]
            sit_out = np.ones(self.boards, dtype=np.uint8)
            sit_out[live] = 0
            groups = np.zeros(self.boards, dtype=np.int32)
            for slot in live:
                groups[slot] = self._mover(self.slots[slot])
            stats["calls"] += 1
            engine.root_eval_groups(self.evaluators, groups, halt=sit_out.astype(bool))
            first = engine.best_moves(self.threshold, False, sit_out)
            one_child = [slot for slot in live if int(first["num_children"][slot]) == 1]
            for slot in live:
                if int(first["num_children"][slot]) != int(engine.root_children[slot]):
                    raise RuntimeError(f"puct_tournament: slot {slot}: the root has {int(first['num_children'][slot])} children "
                                       f"but its expansion drew {int(engine.root_children[slot])} times")
            searching = [slot for slot in live if slot not in set(one_child)]
            if searching:
                # a tree that must not search still does: its game's stream continues where the root expansion left it
                kept = {slot: engine.streams[slot].final_state() for slot in one_child}
                engine.puct_chain_groups(batches, self.evaluators)
                for slot, state in kept.items():
                    engine.set_stream(slot, state)
            moves = engine.best_moves(self.threshold, True, sit_out)
            stats["leaf_evals"] += len(live) + len(searching) * self.visits
            stats["one_child_roots"] += len(one_child)
            self._book(live, moves, stats, on_finished)

    def _book(self, live, moves, stats, on_finished):
        engine = self.engine
        ended = []                                          # (slot, ending, the mover was black)
        for slot in live:
            game, pos = self.slots[slot], int(moves["move"][slot])
            black_moved = len(game.moves) % 2 == 0
            if pos == RESIGN:
                ended.append((slot, "resign", black_moved))
                continue
            game.moves.append((1 if black_moved else 2, pos))
            game.passes = game.passes + 1 if pos == PASS else 0
            stats["moves"] += 1
            if game.passes == 2:
                ended.append((slot, "passes", black_moved))
            elif len(game.moves) >= self.max_moves:
                ended.append((slot, "limit", black_moved))
        if not ended:
            return
        scored = [slot for slot, ending, _ in ended if ending == "passes"]
        scores = {}
        if scored:
            cells, _, _ = engine.read_positions()
            scores = dict(zip(scored, (int(v) for v in engine.count_scores(cells[scored]))))
        for slot, ending, black_moved in ended:
            game = self.slots[slot]
            score = 0.0
            if ending == "resign":
                winner, stone = ("white", Stone.WHITE) if black_moved else ("black", Stone.BLACK)
            elif ending == "passes":
                score = scores[slot] - self.komi
                winner, stone = game_result(score)
            else:
                winner, stone = None, Stone.EMPTY
            state = engine.streams[slot].final_state()
            names = (self.names[game.black], self.names[game.white])
            result = {"index": game.index, "black": names[0], "white": names[1], "winner": winner, "is_resign": ending == "resign",
                      "score": float(score), "moves": len(game.moves), "seed": game.seed,
                      "stream": (np.array(state[1], dtype=np.uint32), int(state[2]))}
            if self.save_dir is not None:
                text = record_text(self.size, names, stone, self.komi, ending == "resign", score, game.moves)
                with open(os.path.join(self.save_dir, f"{game.index}.sgf"), mode="w", encoding="utf-8") as out:
                    out.write(text)
            self.slots[slot] = None
            on_finished(result, game)


def crosstable_of(n_entrants: int, finished) -> list:
    """crosstable[i][j] = {wins, losses, draws, unfinished} of i as black against j as white (None on the diagonal);
    finished: (black index, white index, winner)."""
    table = [[None if i == j else {"wins": 0, "losses": 0, "draws": 0, "unfinished": 0} for j in range(n_entrants)]
             for i in range(n_entrants)]
    for black, white, winner in finished:
        key = {"black": "wins", "white": "losses", "draw": "draws", None: "unfinished"}[winner]
        table[black][white][key] += 1
    return table


def standings_of(names, crosstable) -> list:
    """Per entrant over both colours: games, wins, losses, draws, unfinished and score = wins + draws / 2."""
    n = len(names)
    rows = [{"name": name, "games": 0, "wins": 0, "losses": 0, "draws": 0, "unfinished": 0} for name in names]
    for i in range(n):
        for j in range(n):
            cell = crosstable[i][j]
            if cell is None:
                continue
            total = sum(cell.values())
            for who, won, lost in ((i, "wins", "losses"), (j, "losses", "wins")):
                rows[who]["games"] += total
                rows[who]["wins"] += cell[won]
                rows[who]["losses"] += cell[lost]
                rows[who]["draws"] += cell["draws"]
                rows[who]["unfinished"] += cell["unfinished"]
    for row in rows:
        row["score"] = row["wins"] + 0.5 * row["draws"]
    return rows


def puct_tournament(entrants, visits: int, batch_size: int, games_per_pair: int = 1, size: int = 9, komi: float = 7.0, boards=None,
                    seed_base: int = 0, cgos_mode: bool = False, check_superko: bool = False,
                    resign_threshold: float = RESIGN_THRESHOLD, save_dir=None, device_index: int = 0, _make_engine=None,
                    **not_built) -> dict:
    """A round robin between `entrants` - a list of (name, network), 2 to 64 of them with distinct names - under strict PUCT
    search of `visits` descents in mini-batches of `batch_size` for everybody (see the module docstring for the schedule, the
    game and the call).  One SearchEngine of `boards` slots (default: min(256, games)), tree_size visits + 16; DualNets are
    evaluated on the device and the searches chained in the library, any other evaluator through its host API, mini-batch by
    mini-batch.  Records go to save_dir/<index>.sgf with PB / PW = the names, and save_dir/crosstable.json next to them.

    Not built, and refused with a ValueError: setups that are not strict, reuse_tree, eval_cache, visits or mini-batches per
    entrant, Gumbel search.

    Returns entrants (the names), crosstable (crosstable[i][j] = {wins, losses, draws, unfinished} of i as black against j as
    white), standings (per entrant: games, wins, losses, draws, unfinished, score = wins + draws / 2), elo (per entrant,
    bradley_terry_elo of the pooled results; None where it has no finite rating), results (per game: index, black, white,
    winner, is_resign, score, moves, seed, stream), games, moves, leaf_evals (root evaluations and descents of live games),
    forward_positions (what the launches evaluated), forward_positions_by_entrant, range_fallbacks (of the DualNets:
    bit-identity across launch shapes holds while it is 0), calls, restarts (games started behind the first call),
    one_child_roots, seconds and games_per_second."""
    if not_built:
        raise ValueError("puct_tournament: " + ", ".join(sorted(not_built)) + ": not built - a tournament plays strict PUCT setups "
                         "without reuse_tree, eval_cache, per-entrant searches or Gumbel search")
    if size not in (9, 13, 19):
        raise ValueError(f"puct_tournament: board size {size} is not supported (9, 13 or 19)")
    names, networks = _check_entrants(entrants, size)
    if int(visits) < 1 or int(batch_size) < 1:
        raise ValueError("puct_tournament: visits and batch_size must be at least 1")
    if int(games_per_pair) < 1:
        raise ValueError("puct_tournament: games_per_pair must be >= 1")
    if not 0 <= int(seed_base) < 2 ** 32:
        raise ValueError("puct_tournament: seed_base must be between 0 and 2**32 - 1")
    resign_threshold = float(resign_threshold)
    if math.isnan(resign_threshold) or not 0.0 <= resign_threshold <= 1.0:
        raise ValueError("puct_tournament: resign_threshold must lie in [0, 1] (0 switches resignation off)")
    if boards is not None and boards < 1:
        raise ValueError("puct_tournament: boards must be >= 1")
    pairs = schedule(len(names), int(games_per_pair))
    games = len(pairs)
    boards = max(1, min(boards if boards else 256, games))
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
    queue = []
    for index, (black, white) in enumerate(pairs):
        game = _Game(index, game_seed(seed_base, index))
        game.black, game.white = black, white
        queue.append(game)
    dual = [n for n in {id(n): n for n in networks}.values() if hasattr(n, "range_fallbacks")]
    fallbacks0 = sum(n.range_fallbacks() for n in dual)
    stats = {"moves": 0, "leaf_evals": 0, "calls": 0, "restarts": 0, "one_child_roots": 0}
    results, finished = [], []

    def on_finished(result, game):
        results.append(result)
        finished.append((game.black, game.white, result["winner"]))

    start = time.time()
    table = _Table(names, networks, int(visits), int(batch_size), size, komi, boards, cgos_mode, check_superko, resign_threshold,
                   save_dir, device_index, _make_engine)
    try:
        table.play(queue, stats, on_finished)
        forward = int(getattr(table.engine, "forward_positions", 0))
        by_group = dict(getattr(table.engine, "forward_positions_by_group", {}) or {})
    finally:
        table.close()
    seconds = time.time() - start
    results.sort(key=lambda r: r["index"])
    if len(results) != games:
        raise RuntimeError(f"puct_tournament: {len(results)} of {games} games were played")
    crosstable = crosstable_of(len(names), finished)
    out = {"entrants": names, "crosstable": crosstable, "standings": standings_of(names, crosstable),
           "elo": bradley_terry_elo(pooled_wins(crosstable)), "games": games, "results": results, "moves": stats["moves"],
           "leaf_evals": stats["leaf_evals"], "forward_positions": forward,
           "forward_positions_by_entrant": [int(by_group.get(g, 0)) for g in range(len(names))],
           "range_fallbacks": sum(n.range_fallbacks() for n in dual) - fallbacks0, "calls": stats["calls"],
           "restarts": stats["restarts"], "one_child_roots": stats["one_child_roots"], "seconds": seconds,
           "games_per_second": games / max(seconds, 1e-9)}
    if save_dir is not None:
        with open(os.path.join(save_dir, "crosstable.json"), mode="w", encoding="utf-8") as fp:
            json.dump({k: out[k] for k in ("entrants", "crosstable", "standings", "elo")}, fp)
    return out


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog="python -m tamago_amd.tournament",
                                     description="Round-robin tournament between networks under strict PUCT search.")
    parser.add_argument("--models", nargs="+", required=True, help="model files, one per entrant (2 to 64)")
    parser.add_argument("--names", nargs="+", default=None, help="the entrants' names (default: the files' base names)")
    parser.add_argument("--size", type=int, default=9)
    parser.add_argument("--visits", type=int, required=True)
    parser.add_argument("--batch-size", type=int, default=16)
    parser.add_argument("--games-per-pair", type=int, default=1, help="games per ORDERED pair (black, white)")
    parser.add_argument("--boards", type=int, default=None)
    parser.add_argument("--komi", type=float, default=7.0)
    parser.add_argument("--seed-base", type=int, default=0)
    parser.add_argument("--save-dir", default=None)
    parser.add_argument("--device", type=int, default=0)
    args = parser.parse_args(argv)
    if len(args.models) < 2:
        parser.error("--models takes at least two files")
    if args.names is not None and len(args.names) != len(args.models):
        parser.error("--names takes one name per model")
    return args


def main(argv=None):
    args = parse_args(argv)
    from tamago_amd.nn.utility import load_network
    names = args.names if args.names is not None else [os.path.basename(path) for path in args.models]
    entrants = [(name, load_network(path, True, args.size)) for name, path in zip(names, args.models)]
    out = puct_tournament(entrants, args.visits, args.batch_size, games_per_pair=args.games_per_pair, size=args.size, komi=args.komi,
                          boards=args.boards, seed_base=args.seed_base, save_dir=args.save_dir, device_index=args.device)
    out.pop("results")                                      # (the records are in --save-dir)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
