"""Matches between two engine setups under PUCT search: whole games in lock-step on device-resident boards.

    python -m tamago_amd.match --search puct --black A.bin --white B.bin --games N --visits V --batch-size K
                               [--white-visits V2] [--white-batch-size K2] [--cgos-mode] [--superko] [--swap true] ...
                               [--strict-visits false] [--white-strict-visits false]

A setup is (network, visits, batch_size) and `strict`: the search the GTP engine plays with (MCTSTree.search_best_move), so two
setups may differ in the network, in the visits, only in the mini-batch - the virtual losses a batch of K leaves puts in
flight - or in the visit mode: strict (the default here, the engine's --strict-visits) or not (the engine's default).

A game is defined by the black setup, the white setup, its seed, the komi, the board size, cgos_mode, check_superko and the
resign threshold.  It is the game this loop plays on the reference:

    np.random.seed(seed)                       # once per game: ONE legacy stream, shared by both sides in move order
    board = GoBoard(size, komi, check_superko); color = BLACK
    for ply in range(2 * size * size):         # the self-play limit (selfplay/worker.py:44), as in search_match
        tree.network, tree.batch_size = the mover's
        mode = STRICT_PLAYOUT if the mover's setup is strict else CONSTANT_PLAYOUT
        pos = tree.search_best_move(board, color, TimeManager(mode, the mover's visits))                # mcts/tree.py:57-105
        if pos == RESIGN: the other colour wins by resignation; the move is neither played nor recorded; stop
        board.put_stone(pos, color); two consecutive passes -> score = count_score() - komi, stop
        color = opponent

- the tree rebuilt every move, a root with one child (PASS only) answering PASS without a search and without a draw beyond its
own expansion's, otherwise `visits` descents in mini-batches of batch_size (the last one partial), the first most visited
child, RESIGN when its value is < resign_threshold.  Winner and RE[] follow SelfPlayRecord.to_sgf (the +-0.1 draw band, RE[0]
for a draw and for the move limit); a record is that SGF text without the C[] comments.  A CONSTANT_PLAYOUT search stops
once the runner-up child cannot catch up (time_manager.py:146-163, tested after every full mini-batch that has descents to
follow): the test runs on the device and sets the tree's halt word, which takes the tree out of the lock-step launches that
follow (SearchEngine.puct_chain(early_total=...)).

The boards advance in lock-step and a call moves ONE colour with that colour's network, visits and mini-batch; the calls
alternate, the first is black's, every live game takes part in every call:

    1. tg_search_root_planes, the mover's evaluator, backup                       (SearchEngine.root_eval)
    2. tg_search_best_moves(play = 0): which roots have one child
    3. the mover's mini-batches - puct_chain where can_chain allows, puct_batch otherwise
    4. tg_search_best_moves(play = 1): the move of every live game, decided and played on the device - 32 bytes per tree back
    5. the host's bookkeeping: move lists, passes, the ends of games; count_score of the boards that two passes ended

A strict call's lock-step launches run every tree, so a tree with a one-child root searches although its game does not: the
read-out answers PASS for it whatever that search did to its root, and the game's stream - read after the root expansion - is
put back after the launches (SearchEngine.set_stream: the window in place belonged to the replaced stream and is abandoned).
A call whose mover is not strict halts the one-child roots, the slots of finished games and the empty slots before its
mini-batches (SearchEngine.set_halt): they neither search nor draw, and nothing is put back.  A freed slot
takes its next game (fresh board, the game's seed) only before a black call - slot_may_start(False, mover) - and sits out of
the read-outs until then, as slots with no game left do.

reuse_tree=True (strict setups) plays another game: every game keeps one tree per colour across its moves, as the
GTP engine does under --reuse-tree, and one legacy stream per colour - black RandomState(seed), white RandomState((seed +
2**31) % 2**32).  A leg then holds one engine per colour (_ReuseLeg); a call is

    1. tg_search_root_planes_fresh, the mover's evaluator, backup    (SearchEngine.root_eval_fresh: the fresh trees only)
    2. tg_search_best_moves(play = 0): which roots have one child; those, finished games and empty slots are halted
    3. tg_search_set_budget(visits) and the mover's mini-batches under budgets (puct_chain(budget=True)): a tree that kept
       root visits makes visits - kept descents, and halts once its budget is spent
    4. tg_search_best_moves(play = 0): the moves; tg_search_advance(moves) on BOTH engines - the move played on every root,
       the subtree under it kept where the tree has one
    5. the host's bookkeeping, as above

and its oracle is tests/_puct_reuse_cases.py.
"""
import math
import os
import time
from typing import NamedTuple, Optional, Sequence

import numpy as np

from tamago_amd.board.constant import PASS, RESIGN
from tamago_amd.board.stone import Stone
from tamago_amd.mcts.constant import NN_BATCH_SIZE, PLAYOUTS, RESIGN_THRESHOLD
from tamago_amd.selfplay.match import rating, slot_may_start, tally


class _SetupFields(NamedTuple):
    network: object
    visits: int = PLAYOUTS
    batch_size: int = NN_BATCH_SIZE


class EngineSetup(_SetupFields):
    """One side of a PUCT match: the evaluator (a DualNet, or anything with the DualNet host API) and its search -
    (network, visits, batch_size) as a tuple, and `strict`: True searches every move with exactly `visits` descents
    (STRICT_PLAYOUT), False stops a search early by the reference's default rule (CONSTANT_PLAYOUT)."""

    strict = True                                  # (the class default: what an instance made past __new__ would read)

    def __new__(cls, network, visits: int = PLAYOUTS, batch_size: int = NN_BATCH_SIZE, strict: bool = True):
        self = super().__new__(cls, network, visits, batch_size)
        self.strict = strict
        return self

    # the tuple's own constructors go past __new__: they keep `strict` (_make: a fourth item, if given)
    @classmethod
    def _make(cls, iterable):
        return cls(*iterable)

    def _replace(self, **changes):
        return EngineSetup(**dict(self._asdict(), **changes))

    def _asdict(self):
        return dict(super()._asdict(), strict=self.strict)

    def __eq__(self, other):
        if isinstance(other, EngineSetup) and other.strict != self.strict:
            return False
        return tuple.__eq__(self, other)

    def __ne__(self, other):
        return not self.__eq__(other)

    __hash__ = tuple.__hash__

    def __repr__(self):
        return f"EngineSetup(network={self.network!r}, visits={self.visits!r}, batch_size={self.batch_size!r}, strict={self.strict!r})"


def mini_batches(visits: int, batch_size: int):
    """`visits` descents in mini-batches of batch_size, the last one partial (mcts/tree.py:146-152 with the flush of :84-85)."""
    return [batch_size] * (visits // batch_size) + ([visits % batch_size] if visits % batch_size else [])


def game_result(score: float):
    """(winner, Stone for to_sgf) of a game two passes ended: selfplay/worker.py:82-88, the +-0.1 draw band."""
    if score > 0.1:
        return "black", Stone.BLACK
    if score < -0.1:
        return "white", Stone.WHITE
    return "draw", Stone.OUT_OF_BOARD


def record_text(size: int, names, winner: Stone, komi: float, is_resign: bool, score: float, moves) -> str:
    """SelfPlayRecord.to_sgf without the C[] comments; moves: (colour 1 / 2, padded coordinate) in order."""
    from tamago_amd.board.coordinate import Coordinate
    from tamago_amd.sgf.selfplay_record import SelfPlayRecord
    record = SelfPlayRecord("", Coordinate(size), players=names)
    head, tail = record.to_sgf(winner, komi, is_resign, score).rsplit("\n)", 1)
    body = "".join(f";{'B' if c == 1 else 'W'}[{record.coord.convert_to_sgf_format(p)}]" for c, p in moves)
    return head + body + "\n)" + tail


class _Game:
    def __init__(self, index: int, seed: int):
        self.index, self.seed = index, seed
        self.moves = []                                     # (colour, padded coordinate)
        self.passes = 0


class _Leg:
    """One colour assignment on one lock-step engine of `boards` slots."""

    def __init__(self, black: EngineSetup, white: EngineSetup, size, komi, boards, cgos_mode, check_superko, resign_threshold,
                 save_dir, names, device_index, make_engine=None, poll_every=None, compact_idle=False, eval_caches=None):
        from tamago_amd.board.go_board import GoBoard
        self.poll_every = poll_every
        self.compact_idle = bool(compact_idle)
        self.setups = {Stone.BLACK: black, Stone.WHITE: white}
        self.size, self.boards, self.threshold = size, boards, float(resign_threshold)
        self.save_dir, self.names = save_dir, names
        self.start_board = GoBoard(board_size=size, komi=komi, check_superko=check_superko)
        self.komi = float(self.start_board.get_komi())
        self.max_moves = 2 * size * size
        if make_engine is None:
            from tamago_amd.mcts.engine import SearchEngine, evaluator_for
            self.evaluators = {c: evaluator_for(s.network, device_index, (eval_caches or {}).get(id(s.network))) for c, s in self.setups.items()}
            self.engine = SearchEngine(size, boards, max(black.visits, white.visits) + 16, max(black.batch_size, white.batch_size),
                                       self.evaluators[Stone.BLACK], cgos_mode, check_superko, device_index)
        else:
            self.evaluators = {c: s.network for c, s in self.setups.items()}
            self.engine = make_engine(self)
        self.slots = [None] * boards                        # the _Game in progress
        self.waiting_calls = 0

    def close(self):
        self.engine.close()

    def _start(self, slot: int, game: _Game):
        self.slots[slot] = game
        self.engine.set_root(slot, self.start_board, Stone.BLACK, np.random.RandomState(game.seed).get_state())

    def _search(self, setup: EngineSetup) -> int:
        """The mover's mini-batches; returns the leaf slots per tree that were launched."""
        engine = self.engine
        batches = mini_batches(setup.visits, setup.batch_size)
        if self.compact_idle:
            #  the forward passes cover the trees that search, not the slots: play() reads what was launched off the engine
            run = engine.puct_chain(batches, early_total=None if setup.strict else setup.visits, poll_every=self.poll_every,
                                    compact=True)
            return sum(batches[:run])
        if not setup.strict:
            # time_manager.py:146-163 on the device, where MCTSTree.search tests it: behind every full mini-batch that has
            # descents to follow
            return sum(batches[:engine.puct_chain(batches, early_total=setup.visits, poll_every=self.poll_every)])
        if engine.can_chain(setup.visits):
            engine.puct_chain(batches)
        else:
            for leaves in batches:
                engine.ensure_capacity(leaves)
                engine.puct_batch(leaves)
        return setup.visits

    def play(self, queue, stats, on_finished):
        """The games of `queue` (_Game objects, in order) to their ends."""
        engine = self.engine
        queue = list(queue)
        mover = Stone.BLACK
        idle_from = None
        while queue or any(g is not None for g in self.slots):
            if slot_may_start(False, mover):
                for slot in range(self.boards):
                    if self.slots[slot] is None and queue:
                        self._start(slot, queue.pop(0))
            live = [slot for slot, g in enumerate(self.slots) if g is not None]
            parked = self.boards - len(live) if queue else 0          # slots that wait for a call they may start on
            stats["calls"] += 1
            stats["slot_calls"] += self.boards
            stats["parked_slot_calls"] += parked
            if live:
                setup = self.setups[mover]
                sit_out = np.ones(self.boards, dtype=np.uint8)
                sit_out[live] = 0
                engine.evaluator = self.evaluators[mover]
                if idle_from is not None:
                    stats["between_calls_seconds"] += time.perf_counter() - idle_from
                engine.root_eval(use_logit=False)
                first = engine.best_moves(self.threshold, False, sit_out)
                one_child = [slot for slot in live if int(first["num_children"][slot]) == 1]
                for slot in live:
                    if int(first["num_children"][slot]) != int(engine.root_children[slot]):
                        raise RuntimeError(f"puct_match: slot {slot}: the root has {int(first['num_children'][slot])} children "
                                           f"but its expansion drew {int(engine.root_children[slot])} times")
                forward = self.boards
                passing = set(one_child)
                searching = [slot for slot in live if slot not in passing]
                launched0 = engine.forward_positions if self.compact_idle else 0      # (compact: the engine counts what it launches)
                if searching and setup.strict:
                    # a tree that must not search still does: its game's stream continues where the root expansion left it
                    kept = {slot: engine.streams[slot].final_state() for slot in one_child}
                    if self.compact_idle and sit_out.any():
                        engine.set_halt(sit_out.astype(bool))       # slots without a game: halted, and compacted away
                    self._search(setup)
                    for slot, state in kept.items():
                        engine.set_stream(slot, state)
                    forward += engine.forward_positions - launched0 if self.compact_idle else self.boards * setup.visits
                    stats["leaf_evals"] += len(searching) * setup.visits
                elif searching:
                    # trees that must not search do not: halted, they take no draw, and a searching tree halts where its
                    # search stops early
                    idle = sit_out.astype(bool)
                    idle[one_child] = True
                    if idle.any():
                        engine.set_halt(idle)
                    slots = self._search(setup)
                    forward += engine.forward_positions - launched0 if self.compact_idle else self.boards * slots
                moves = engine.best_moves(self.threshold, True, sit_out)
                if searching and not setup.strict:
                    stats["leaf_evals"] += int(sum(int(moves["node_visits"][slot]) for slot in searching))
                idle_from = time.perf_counter()
                stats["leaf_evals"] += len(live)
                stats["forward_positions"] += forward
                stats["one_child_roots"] += len(one_child)
                self._book(mover, live, moves, stats, on_finished)
            mover = Stone.get_opponent_color(mover)

    def _book(self, mover, live, moves, stats, on_finished):
        engine = self.engine
        ended = []                                          # (slot, ending)
        for slot in live:
            game, pos = self.slots[slot], int(moves["move"][slot])
            if pos == RESIGN:
                ended.append((slot, "resign"))
                continue
            game.moves.append((1 if mover == Stone.BLACK else 2, pos))
            game.passes = game.passes + 1 if pos == PASS else 0
            stats["moves"] += 1
            if game.passes == 2:
                ended.append((slot, "passes"))
            elif len(game.moves) >= self.max_moves:
                ended.append((slot, "limit"))
        if not ended:
            return
        scored = [slot for slot, ending in ended if ending == "passes"]
        scores = {}
        if scored:
            cells, _, _ = engine.read_positions()
            scores = dict(zip(scored, (int(v) for v in engine.count_scores(cells[scored]))))
        for slot, ending in ended:
            game = self.slots[slot]
            score = 0.0
            if ending == "resign":
                winner, stone = ("white", Stone.WHITE) if mover == Stone.BLACK else ("black", Stone.BLACK)
            elif ending == "passes":
                score = scores[slot] - self.komi
                winner, stone = game_result(score)
            else:
                winner, stone = None, Stone.EMPTY
            state = engine.streams[slot].final_state()
            result = {"index": game.index, "winner": winner, "is_resign": ending == "resign", "score": float(score),
                      "moves": len(game.moves), "seed": game.seed,
                      "stream": (np.array(state[1], dtype=np.uint32), int(state[2]))}
            result.update(self._more_result(slot))
            if self.save_dir is not None:
                text = record_text(self.size, self.names, stone, self.komi, ending == "resign", score, game.moves)
                with open(os.path.join(self.save_dir, f"{game.index}.sgf"), mode="w", encoding="utf-8") as out:
                    out.write(text)
            self.slots[slot] = None
            stats["games"] += 1
            on_finished(result)


    def _more_result(self, slot: int) -> dict:
        return {}


def white_seed(seed: int) -> int:
    """The seed of white's stream in a game with tree reuse (black's is the game's seed)."""
    return (int(seed) + 2 ** 31) % 2 ** 32


class _ReuseLeg(_Leg):
    """One colour assignment with tree reuse: one lock-step engine of `boards` slots PER COLOUR on the same
    stream, each with its colour's evaluator, visits and mini-batch and its own legacy stream per game.  A call launches the
    mover's engine only; the moves it decides advance the roots of BOTH engines on the device (SearchEngine.advance), so
    every tree sees every move of its game and keeps the subtree under it where it has one."""

    def __init__(self, black: EngineSetup, white: EngineSetup, size, komi, boards, cgos_mode, check_superko, resign_threshold,
                 save_dir, names, device_index, make_engine=None, poll_every=None, compact_idle=False, eval_caches=None):
        from tamago_amd.board.go_board import GoBoard
        from tamago_amd.mcts.engine import SearchEngine, evaluator_for
        if make_engine is not None:
            raise ValueError("puct_match: reuse_tree builds its own engines")
        self.poll_every = poll_every
        self.compact_idle = bool(compact_idle)
        self.setups = {Stone.BLACK: black, Stone.WHITE: white}
        self.size, self.boards, self.threshold = size, boards, float(resign_threshold)
        self.save_dir, self.names = save_dir, names
        self.start_board = GoBoard(board_size=size, komi=komi, check_superko=check_superko)
        self.komi = float(self.start_board.get_komi())
        self.max_moves = 2 * size * size
        self.evaluators = {c: evaluator_for(s.network, device_index, (eval_caches or {}).get(id(s.network))) for c, s in self.setups.items()}
        # (a kept subtree holds at most one node per kept visit and the root: kept nodes + owed descents <= visits + 1)
        self.engines = {c: SearchEngine(size, boards, s.visits + 16, s.batch_size, self.evaluators[c], cgos_mode, check_superko,
                                        device_index) for c, s in self.setups.items()}
        self.engine = self.engines[Stone.BLACK]             # (_book reads the positions and black's streams off it)
        self.kept = {c: np.full(boards, -1, dtype=np.int64) for c in self.setups}     # root visits each tree kept, -1: fresh
        self.slots = [None] * boards
        self.waiting_calls = 0

    def close(self):
        for engine in self.engines.values():
            engine.close()

    def _start(self, slot: int, game: _Game):
        self.slots[slot] = game
        for color, seed in ((Stone.BLACK, game.seed), (Stone.WHITE, white_seed(game.seed))):
            self.engines[color].set_root(slot, self.start_board, Stone.BLACK, np.random.RandomState(seed).get_state())
            self.kept[color][slot] = -1

    def _more_result(self, slot: int) -> dict:
        state = self.engines[Stone.WHITE].streams[slot].final_state()
        return {"stream_white": (np.array(state[1], dtype=np.uint32), int(state[2]))}

    def play(self, queue, stats, on_finished):
        queue = list(queue)
        mover = Stone.BLACK
        idle_from = None
        for key in ("reused_searches", "fresh_searches", "kept_visits", "budget_visits", "advance_seconds", "root_fresh_seconds"):
            stats.setdefault(key, 0)
        while queue or any(g is not None for g in self.slots):
            if slot_may_start(False, mover):
                for slot in range(self.boards):
                    if self.slots[slot] is None and queue:
                        self._start(slot, queue.pop(0))
            live = [slot for slot, g in enumerate(self.slots) if g is not None]
            parked = self.boards - len(live) if queue else 0
            stats["calls"] += 1
            stats["slot_calls"] += self.boards
            stats["parked_slot_calls"] += parked
            if live:
                setup, engine = self.setups[mover], self.engines[mover]
                kept = self.kept[mover]
                sit_out = np.ones(self.boards, dtype=np.uint8)
                sit_out[live] = 0
                if idle_from is not None:
                    stats["between_calls_seconds"] += time.perf_counter() - idle_from
                launched0 = engine.forward_positions
                t0 = time.perf_counter()
                engine.root_eval_fresh(use_logit=False)
                first = engine.best_moves(self.threshold, False, sit_out)
                stats["root_fresh_seconds"] += time.perf_counter() - t0
                one_child = [slot for slot in live if int(first["num_children"][slot]) == 1]
                for slot in live:
                    if int(first["num_children"][slot]) != int(engine.root_children[slot]):
                        raise RuntimeError(f"puct_match: slot {slot}: the root has {int(first['num_children'][slot])} children "
                                           f"but its expansion or advance reported {int(engine.root_children[slot])}")
                passing = set(one_child)
                searching = [slot for slot in live if slot not in passing]
                if searching:
                    # trees that must not search do not: halted, they take no draw; a searching tree owes what its budget
                    # leaves of `visits` and halts (budget rule) once that is spent
                    idle = sit_out.astype(bool)
                    idle[one_child] = True
                    if idle.any():
                        engine.set_halt(idle)
                    # (an idle tree's total is 1: it owes nothing the pool would have to hold)
                    engine.set_budget(np.where(idle, 1, setup.visits))
                    engine.puct_chain(mini_batches(setup.visits, setup.batch_size), budget=True, poll_every=self.poll_every,
                                      compact=self.compact_idle)
                moves = engine.best_moves(self.threshold, False, sit_out)
                played = np.full(self.boards, -1, dtype=np.int32)
                for slot in live:
                    if int(moves["move"][slot]) != RESIGN:
                        played[slot] = int(moves["move"][slot])
                t0 = time.perf_counter()
                for color, other in self.engines.items():
                    records = other.advance(played)
                    if (played >= 0).any():
                        # every tree that searches again was advanced here or starts fresh; the others are halted until
                        # their slot takes a new game, so the engine's bound need not count them (it would only ever grow
                        # for a slot that sits out, and end the chained launches for the whole leg)
                        other.node_bound = max(1, int(records["kept_nodes"][played >= 0].max()))
                    self.kept[color] = np.where(played >= 0, records["kept_visits"].astype(np.int64), self.kept[color])
                stats["advance_seconds"] += time.perf_counter() - t0
                idle_from = time.perf_counter()
                for slot in searching:
                    had = int(kept[slot])
                    stats["fresh_searches" if had < 0 else "reused_searches"] += 1
                    stats["kept_visits"] += max(had, 0)
                    stats["budget_visits"] += setup.visits
                    stats["leaf_evals"] += max(0, int(moves["node_visits"][slot]) - max(had, 0))
                stats["leaf_evals"] += sum(1 for slot in live if int(kept[slot]) < 0)
                stats["forward_positions"] += engine.forward_positions - launched0
                stats["one_child_roots"] += len(one_child)
                self._book(mover, live, moves, stats, on_finished)
            mover = Stone.get_opponent_color(mover)


def _check_setup(setup, which: str, size: int) -> EngineSetup:
    if not isinstance(setup, EngineSetup):
        raise ValueError(f"puct_match: {which} must be an EngineSetup(network, visits, batch_size)")
    if not isinstance(setup.strict, bool):
        raise ValueError(f"puct_match: {which}: strict must be True or False")
    if int(setup.visits) < 1 or int(setup.batch_size) < 1:
        raise ValueError(f"puct_match: {which}: visits and batch_size must be at least 1")
    net_size = getattr(setup.network, "board_size", None)
    if net_size is not None and net_size != size:
        raise ValueError(f"puct_match: {which}: network is built for {net_size}x{net_size}, the match is {size}x{size}")
    return EngineSetup(setup.network, int(setup.visits), int(setup.batch_size), setup.strict)


def puct_match(setup_a: EngineSetup, setup_b: EngineSetup, games: int, size: int = 9, komi: float = 7.0, boards=None,
               swap: bool = False, seeds: Sequence[int] = None, cgos_mode: bool = False, check_superko: bool = False,
               resign_threshold: float = RESIGN_THRESHOLD, save_dir=None, names=("A", "B"), device_index: int = 0,
               _make_engine=None, poll_every=None, compact_idle: bool = False, reuse_tree: bool = False,
               eval_cache: Optional[int] = None) -> dict:
    """setup_a against setup_b under PUCT search (see the module docstring for the game): `games` games with A as black and,
    with swap, `games` more with A as white.

    Game g of a leg draws from the legacy stream seeded with seeds[g] (default: g); the swapped leg replays the same seeds
    with the setups exchanged.  Records go to save_dir/<index>.sgf, index g for the first leg and games + g for the swapped
    one, with PB / PW = `names` in the leg's colours; no save_dir, no files.  resign_threshold 0.0 switches resignation off.
    poll_every: for calls whose mover is not strict, the mini-batches between two looks at whether a tree is still searching
    (SearchEngine.puct_chain; None: its default, 0: never) - a call can end early only where it looks, so with fewer mini-batches
    per move than poll_every the halted trees save selection work but every call runs all its mini-batches; the games do not
    depend on it.  One lock-step engine of `boards` slots (default: min(256, games)) per leg; DualNets are evaluated on the device, any
    other evaluator through its host API, a mixed pair too.
    compact_idle: trees that do not search are compacted out of the forward passes - in calls that are not strict
    the halted ones (slots without a game, one-child roots, trees whose search stopped early, as of the last look), in strict
    calls the slots without a game, which are halted for it (one-child roots search on, as above).  Same games, records and
    streams; forward_positions reports what was really launched.

    reuse_tree (both setups strict, else ValueError): every game keeps one search tree per colour across its
    moves, as the GTP engine does under --reuse-tree - each searched only by its own network, advanced by every move of the
    game on the device, topped up to the colour's visits where it kept a subtree.  ANOTHER game than without: each colour
    draws from a stream of its own (black's seeded with the game's seed, white's with (seed + 2**31) % 2**32), a reused root
    draws nothing, and the searches differ.  A result then also carries stream_white, and the return value reused_searches,
    fresh_searches, kept_share (mean share of the visits a search found kept), advance_seconds and root_fresh_seconds.

    eval_cache (entries, None / 0: off): every distinct network object gets an evaluation cache of that many
    entries for the whole match - two setups on the same network share one - and positions whose outputs it holds are not
    evaluated again.  The searches go mini-batch by mini-batch then (a cached evaluator is not chained).  Same games, records
    and streams; forward_positions stays what the engine handed over, evaluated_positions reports what the networks were
    really given, and eval_cache_stats the caches' counters (nn/eval_cache.py STAT_NAMES, entries, caches).

    Returns search_match's keys where they apply - games, wins_a, wins_b, draws, unfinished, as_black / as_white,
    resignations, mean_length, decided, score_a, elo, elo_interval, leaf_evals (root evaluations and descents of live games),
    forward_positions (what the launches evaluated, parked and pass-only trees included), moves, range_fallbacks (of the
    DualNets: bit-identity across launch shapes holds while it is 0), calls, slot_calls, parked_slot_calls, seconds,
    games_per_second, results - and one_child_roots (moves answered PASS without a search) and between_calls_seconds (host
    time from a call's last read-out to the next call's root launch).  A per-game result carries index, winner, is_resign,
    score, moves, seed, a_is_black and `stream`: the MT19937 state (key, position) of the game's stream at its end."""
    if games < 1:
        raise ValueError("puct_match: games must be >= 1")
    if size not in (9, 13, 19):
        raise ValueError(f"puct_match: board size {size} is not supported (9, 13 or 19)")
    setup_a, setup_b = _check_setup(setup_a, "setup_a", size), _check_setup(setup_b, "setup_b", size)
    if reuse_tree and not (setup_a.strict and setup_b.strict):
        raise ValueError("puct_match: reuse_tree needs strict setups (a reused root that already decides the move is not built)")
    seeds = [int(s) for s in seeds] if seeds is not None else list(range(games))
    if len(seeds) != games:
        raise ValueError("puct_match: seeds takes one entry per game")
    if any(s < 0 or s >= 2 ** 32 for s in seeds):
        raise ValueError("puct_match: seeds must be between 0 and 2**32 - 1")
    if len(names) != 2:
        raise ValueError("puct_match: names takes the two players' names")
    resign_threshold = float(resign_threshold)
    if math.isnan(resign_threshold) or not 0.0 <= resign_threshold <= 1.0:
        raise ValueError("puct_match: resign_threshold must lie in [0, 1] (0 switches resignation off)")
    if boards is not None and boards < 1:
        raise ValueError("puct_match: boards must be >= 1")
    boards = max(1, min(boards if boards else 256, games))
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
    dual = [n for n in {id(s.network): s.network for s in (setup_a, setup_b)}.values() if hasattr(n, "range_fallbacks")]
    fallbacks0 = sum(n.range_fallbacks() for n in dual)
    stats = {"games": 0, "moves": 0, "leaf_evals": 0, "forward_positions": 0, "calls": 0, "slot_calls": 0,
             "parked_slot_calls": 0, "one_child_roots": 0, "between_calls_seconds": 0.0}
    results = []
    caches, evaluated = {}, 0
    if eval_cache and _make_engine is None:
        from tamago_amd.nn.eval_cache import caches_for
        caches = caches_for((setup_a.network, setup_b.network), size, int(eval_cache), device_index)
    start = time.time()
    try:
        for leg, a_is_black in enumerate((True, False) if swap else (True,)):
            black, white = (setup_a, setup_b) if a_is_black else (setup_b, setup_a)
            leg_names = (names[0], names[1]) if a_is_black else (names[1], names[0])
            runner = (_ReuseLeg if reuse_tree else _Leg)(black, white, size, komi, boards, cgos_mode, check_superko, resign_threshold,
                                                         save_dir, leg_names, device_index, _make_engine, poll_every, compact_idle,
                                                         **(dict(eval_caches=caches) if caches else {}))
            try:
                runner.play([_Game(leg * games + g, seeds[g]) for g in range(games)], stats,
                            lambda result, a_is_black=a_is_black: results.append(dict(result, a_is_black=a_is_black)))
            finally:
                runner.close()
                if caches:
                    evaluated += sum(sum(e.batches) for e in runner.evaluators.values())
        cache_stats = None
        if caches:
            from tamago_amd.nn.eval_cache import total_stats
            cache_stats = total_stats(list(caches.values()))
    finally:
        for cache in caches.values():
            cache.close()
    seconds = time.time() - start
    results.sort(key=lambda r: r["index"])
    out = tally(results)
    if out["games"] != games * (2 if swap else 1):
        raise RuntimeError(f"puct_match: {out['games']} of {games * (2 if swap else 1)} games were played")
    out.update(rating(out["wins_a"], out["wins_b"], out["draws"]))
    out.update(leaf_evals=stats["leaf_evals"], forward_positions=stats["forward_positions"], moves=stats["moves"],
               range_fallbacks=sum(n.range_fallbacks() for n in dual) - fallbacks0, calls=stats["calls"],
               slot_calls=stats["slot_calls"], parked_slot_calls=stats["parked_slot_calls"],
               one_child_roots=stats["one_child_roots"], between_calls_seconds=stats["between_calls_seconds"],
               seconds=seconds, games_per_second=out["games"] / max(seconds, 1e-9), results=results)
    if reuse_tree:
        out.update(reused_searches=stats["reused_searches"], fresh_searches=stats["fresh_searches"],
                   kept_share=stats["kept_visits"] / max(stats["budget_visits"], 1), advance_seconds=stats["advance_seconds"],
                   root_fresh_seconds=stats["root_fresh_seconds"])
    if caches:
        out.update(evaluated_positions=evaluated, eval_cache_stats=cache_stats)
    return out
