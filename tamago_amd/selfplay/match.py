"""Matches between two networks under Gumbel search: the self-play loop with one evaluator per colour.

    python -m tamago_amd.match --black A.bin --white B.bin --games N [--size 9] [--visits 16] [--boards B] [--komi 7.0]
                               [--swap true] [--save-dir DIR] [--unique-leaves true]
                               [--search puct --visits N --batch-size K [--white-visits N2] [--white-batch-size K2]
                                [--cgos-mode] [--superko]]       (PUCT matches: selfplay/puct_match.py; the default
                                                                  --search gumbel is the match described here)

prints one JSON line: wins of A and of B, draws, unfinished games, the same split by A's colour, resignations, mean length,
leaf evaluations, A's score, an Elo difference with a 95 % interval, games per second.

A game is defined by the black evaluator X, the white evaluator Y, its seed, never_resign, the visits, the komi and the board
size: it is the game the reference's selfplay_worker loop (selfplay/worker.py:44-90) plays after np.random.seed(seed) with
mcts.network = X for every black move and Y for every white move - the tree rebuilt every move, the ONE legacy stream shared by
both sides in move order, the worker's resign rule, two-pass end with count_score, maximum length 2 * S * S and SGF text.  With
X is Y it is the self-play game of that seed; the record differs from a self-play record in PB[] / PW[] only.

The boards advance in lock-step (selfplay/worker.py: _LockStep), and a lock-step call moves ONE colour: its phases run on the
mover's network.  So the calls alternate between the colours, and a freed slot takes its next game only on a call it may start
on (slot_may_start) - the one place where a match costs more than self-play.
"""
import argparse
import json
import math
import os
import time
from typing import Optional, Sequence

from tamago_amd.board.stone import Stone
from tamago_amd.selfplay.worker import SELF_PLAY_VISITS


def _flag(text: str) -> bool:
    return text.lower() in ("1", "true", "yes")


def handle_is_chained(lib, handle=None) -> bool:
    """tg_selfplay_chained: the scheme the handle's one-call moves run in, asked of the library - the only reader of its
    knobs - before the first move (the handle keeps to the answer).  handle None: what a new handle would be told."""
    import ctypes
    from tamago_amd import lib as _lib
    chained = ctypes.c_int(0)
    _lib.check(lib.tg_selfplay_chained(handle, ctypes.byref(chained)), "tg_selfplay_chained")
    return chained.value != 0


def first_mover(chained: bool):
    """The colour that "moves" in a handle's first call.  Chained scheme: the first call only evaluates the roots of the games
    just started, with the network of the NEXT call's mover - black -, so it counts as white's.  Round-trip and phase-by-phase
    schemes: a started game is searched at once, so the first call is black's."""
    return Stone.WHITE if chained else Stone.BLACK


def slot_may_start(chained: bool, next_mover) -> bool:
    """May a slot whose game has ended take its next game before the coming call, in which `next_mover` moves?  A new game
    has black to move, and a call evaluates with the mover's network only (the chained scheme's closing root evaluation: with
    the OTHER colour's).
      chained scheme: a started slot sits out the coming call, whose chain evaluates its root for the call after - that
        evaluation must be black's, so the coming call must be white's.  A game that ended on black's call is therefore
        restarted at once; one that ended on white's call stays parked for one extra call.
      round-trip and phase-by-phase schemes: a started slot is searched in the coming call, which must be black's: a game that
        ended on white's call restarts at once, one that ended on black's call waits one call.
    The library enforces the consequence (tg_selfplay_play_move2: TG_ERR_STATE); both drivers in this module ask here."""
    return next_mover == (Stone.WHITE if chained else Stone.BLACK)


class _Turns:
    """Whose call is next in a leg, and the two questions the drivers ask of it."""

    def __init__(self, chained: bool):
        self.chained = chained
        self.mover = first_mover(chained)                   # the colour that moves in the coming call

    @property
    def other(self):
        return Stone.get_opponent_color(self.mover)

    def flip(self):
        self.mover = self.other

    def may_start(self) -> bool:
        return slot_may_start(self.chained, self.mover)


def tally(results) -> dict:
    """Counts from per-game results ({"winner": "black" | "white" | "draw" | None, "is_resign", "moves", "a_is_black"}):
    wins_a / wins_b / draws / unfinished (None: the move limit), the same for A as black and A as white, resignations and the
    mean length."""
    keys = ("wins_a", "wins_b", "draws", "unfinished")
    out = {"games": 0, **{k: 0 for k in keys}, "as_black": {k: 0 for k in keys}, "as_white": {k: 0 for k in keys},
           "resignations": 0}
    lengths = 0
    for game in results:
        side = out["as_black" if game["a_is_black"] else "as_white"]
        if game["winner"] is None:
            key = "unfinished"
        elif game["winner"] == "draw":
            key = "draws"
        else:
            key = "wins_a" if (game["winner"] == "black") == game["a_is_black"] else "wins_b"
        out[key] += 1
        side[key] += 1
        out["games"] += 1
        out["resignations"] += 1 if game["is_resign"] else 0
        lengths += game["moves"]
    out["mean_length"] = lengths / out["games"] if out["games"] else 0.0
    return out


def _elo(score: float) -> Optional[float]:
    """400 log10(p / (1 - p)); None at 0 or 1, where the difference is unbounded."""
    if not 0.0 < score < 1.0:
        return None
    return 400.0 * math.log10(score / (1.0 - score))


def rating(wins_a: int, wins_b: int, draws: int) -> dict:
    """A's score over the decided games, (wins_a + draws / 2) / decided, its Elo difference and the normal-approximation 95 %
    interval: the per-game scores 1, 1/2, 0 have the sample variance v, the mean the standard error sqrt(v / decided), and the
    interval's ends are the Elo of score -+ 1.96 standard errors (None where an end leaves (0, 1))."""
    decided = wins_a + wins_b + draws
    if decided == 0:
        return {"decided": 0, "score_a": None, "elo": None, "elo_interval": [None, None]}
    score = (wins_a + 0.5 * draws) / decided
    variance = max((wins_a + 0.25 * draws) / decided - score * score, 0.0)
    half = 1.96 * math.sqrt(variance / decided)
    return {"decided": decided, "score_a": score, "elo": _elo(score), "elo_interval": [_elo(score - half), _elo(score + half)]}


def _play_leg(black, white, queue, seeds, size, visits, komi, boards, save_dir, names, unique_leaves, device_index, stats,
              on_finished):
    """One colour assignment: the games of `queue` ((index, never_resign) pairs) on one lock-step group of `boards` slots."""
    import torch
    from tamago_amd import lib as _lib
    from tamago_amd.mcts.engine import DeviceEvaluator, evaluator_for
    from tamago_amd.nn.network.dual_net import DualNet
    from tamago_amd.selfplay.worker import _LockStep, _PhaseByPhaseMove
    one_call = isinstance(black, DualNet) and isinstance(white, DualNet)
    nets = {Stone.BLACK: black, Stone.WHITE: white}
    evaluators = {c: DeviceEvaluator(n) if one_call else evaluator_for(n, device_index) for c, n in nets.items()}
    queue = list(queue)
    group = _LockStep(save_dir, evaluators[Stone.BLACK], size, visits, boards, seeds, device_index,
                      lambda: queue.pop(0) if queue else None, unique_leaves, komi=komi, players=names,
                      games_left=lambda: bool(queue), on_finished=on_finished)
    engine, lib, handle = group.engine, group.lib, group.handle
    try:
        # the phase-by-phase path searches a started slot at once, as the round-trip scheme does; the one-call path runs the
        # scheme the handle says it runs
        turns = _Turns(one_call and handle_is_chained(lib, handle))
        group.may_start = turns.may_start
        group.fill()                                        # (slot_may_start holds for first_mover)
        if one_call:
            policy, value = group.outputs()
            while group.live > 0:
                _lib.check(lib.tg_selfplay_play_move2(handle, nets[turns.mover].handle, nets[turns.other].handle,
                                                      engine.planes.data_ptr(), policy.data_ptr(), value.data_ptr(),
                                                      engine._stream(), group.finished.ctypes.data, group.counts.ctypes.data),
                           "tg_selfplay_play_move2")
                turns.flip()
                group.after_move(stats)
        else:
            move = _PhaseByPhaseMove(group, unique_leaves)
            while group.live > 0:
                engine.evaluator = evaluators[turns.mover]
                move.play(stats)
                turns.flip()
                group.after_move(stats)
        torch.cuda.synchronize(engine.device)
        stats["calls"] += group.calls
        stats["slot_calls"] += group.calls * boards
        stats["parked_slot_calls"] += group.waited_calls
    finally:
        group.close(stats)


def search_match(net_a, net_b, games: int, size: int = 9, visits: int = SELF_PLAY_VISITS, komi: float = 7.0, boards=None,
                 swap: bool = False, seeds: Sequence[int] = None, never_resign_flags: Sequence[bool] = None, save_dir=None,
                 names=("A", "B"), unique_leaves: bool = False, device_index: int = 0, groups: int = 1, lanes: int = 1) -> dict:
    """net_a against net_b under Gumbel search with `visits` simulations per move: `games` games with A as black and, with
    swap, `games` more with A as white.

    Game g of a leg draws from the legacy stream seeded with seeds[g] (default: g); the swapped leg uses the same seeds, so each
    seed is played from both sides.  never_resign_flags[g] (default: resignation allowed everywhere - self-play's 10 % draw
    exists for training data) holds for both legs as well.  Records go to save_dir/<index>.sgf, index g for the first leg and
    games + g for the swapped one, with PB / PW = `names` in the leg's colours; no save_dir, no files.

    Two DualNets play through tg_selfplay_play_move2; any other pair (a mixed one too) is driven phase by phase with the
    engine's evaluator switched to the mover's.  One lock-step group, one lane (the library's sub-groups inside a call are its
    own business): `groups` / `lanes` above 1 are refused.  TG_SP_LANES is not consulted.

    Returns wins_a, wins_b, draws, unfinished, as_black / as_white (the same four for A's colour), resignations, mean_length,
    leaf_evals, forward_positions, range_fallbacks, seconds, games_per_second, score_a, elo, elo_interval, the per-game
    `results` and the lock-step calls: calls, slot_calls, parked_slot_calls (slots that waited for a call they may start on)."""
    if groups > 1 or lanes > 1:
        raise ValueError("search_match: a match runs as one lock-step group and one lane (groups / lanes > 1 are not supported)")
    if games < 1:
        raise ValueError("search_match: games must be >= 1")
    seeds = list(seeds) if seeds is not None else list(range(games))
    flags = [bool(f) for f in never_resign_flags] if never_resign_flags is not None else [False] * games
    if len(seeds) != games or len(flags) != games:
        raise ValueError("search_match: seeds and never_resign_flags take one entry per game")
    boards = max(1, min(boards if boards else 256, games))
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
    dual = [n for n in {id(net_a): net_a, id(net_b): net_b}.values() if hasattr(n, "range_fallbacks")]
    fallbacks0 = sum(n.range_fallbacks() for n in dual)
    stats = {"games": 0, "moves": 0, "leaf_evals": 0, "forward_positions": 0, "calls": 0, "slot_calls": 0, "parked_slot_calls": 0}
    results = []
    start = time.time()
    for leg, a_is_black in enumerate((True, False) if swap else (True,)):
        black, white = (net_a, net_b) if a_is_black else (net_b, net_a)
        leg_names = (names[0], names[1]) if a_is_black else (names[1], names[0])
        indices = [leg * games + g for g in range(games)]

        def on_finished(result, a_is_black=a_is_black, leg=leg):
            results.append(dict(result, a_is_black=a_is_black, seed=seeds[result["index"] - leg * games]))

        _play_leg(black, white, list(zip(indices, flags)), dict(zip(indices, seeds)), size, visits, komi, boards, save_dir,
                  leg_names, unique_leaves, device_index, stats, on_finished)
    seconds = time.time() - start
    results.sort(key=lambda r: r["index"])
    out = tally(results)
    if out["games"] != games * (2 if swap else 1):
        raise RuntimeError(f"search_match: {out['games']} of {games * (2 if swap else 1)} games were played")
    out.update(rating(out["wins_a"], out["wins_b"], out["draws"]))
    out.update(leaf_evals=stats["leaf_evals"], forward_positions=stats["forward_positions"], moves=stats["moves"],
               range_fallbacks=sum(n.range_fallbacks() for n in dual) - fallbacks0, calls=stats["calls"],
               slot_calls=stats["slot_calls"], parked_slot_calls=stats["parked_slot_calls"], seconds=seconds,
               games_per_second=out["games"] / seconds, results=results)
    return out


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog="python -m tamago_amd.match")
    parser.add_argument("--black", required=True, help="model file of network A (black in the first leg)")
    parser.add_argument("--white", required=True, help="model file of network B")
    parser.add_argument("--games", type=int, required=True)
    parser.add_argument("--size", type=int, default=9)
    parser.add_argument("--visits", type=int, default=SELF_PLAY_VISITS)
    parser.add_argument("--boards", type=int, default=None)
    parser.add_argument("--komi", type=float, default=7.0)
    parser.add_argument("--swap", type=_flag, default=False)
    parser.add_argument("--save-dir", default=None)
    parser.add_argument("--unique-leaves", type=_flag, default=False)
    # --search puct: whole games under the PUCT search the GTP engine plays with (selfplay/puct_match.py), --visits strict
    # visits per move in mini-batches of --batch-size; white's may differ
    parser.add_argument("--search", choices=("gumbel", "puct"), default="gumbel")
    parser.add_argument("--batch-size", type=int, default=None, help="puct: leaves per mini-batch (default 16)")
    parser.add_argument("--white-visits", type=int, default=None, help="puct: white's visits (default: --visits)")
    parser.add_argument("--white-batch-size", type=int, default=None, help="puct: white's mini-batch (default: --batch-size)")
    parser.add_argument("--cgos-mode", action="store_true", help="puct: the reference's cgos_mode selection")
    parser.add_argument("--superko", action="store_true", help="puct: boards that check positional superko")
    parser.add_argument("--strict-visits", type=_flag, default=None,
                        help="puct: true (default) searches every move with exactly --visits descents, false stops a search "
                             "once the runner-up cannot catch up (the GTP engine's default)")
    parser.add_argument("--white-strict-visits", type=_flag, default=None, help="puct: white's (default: --strict-visits)")
    parser.add_argument("--poll-every", type=int, default=None,
                        help="puct, not strict: mini-batches between two looks at whether a search is still running (0: never)")
    parser.add_argument("--compact-idle", action="store_true",
                        help="puct: leave trees that do not search (finished games, empty slots, halted trees) out of the forward "
                             "passes; same games")
    parser.add_argument("--reuse-tree", action="store_true",
                        help="puct, strict: keep each colour's search tree across the moves of a game (the GTP engine's "
                             "--reuse-tree): one tree per game and colour, advanced by every move; other games than without")
    parser.add_argument("--eval-cache", type=int, default=None, metavar="N",
                        help="puct: an evaluation cache of N entries per network serves positions that were evaluated before "
                             "(the searches go mini-batch by mini-batch); same games")
    args = parser.parse_args(argv)
    if args.eval_cache is not None and args.eval_cache < 1:
        parser.error("--eval-cache: at least 1 entry")
    if args.search == "gumbel":
        given = [flag for flag, value in (("--batch-size", args.batch_size), ("--white-visits", args.white_visits),
                                          ("--white-batch-size", args.white_batch_size), ("--cgos-mode", args.cgos_mode),
                                          ("--superko", args.superko), ("--strict-visits", args.strict_visits is not None),
                                          ("--white-strict-visits", args.white_strict_visits is not None),
                                          ("--poll-every", args.poll_every is not None),
                                          ("--compact-idle", args.compact_idle), ("--reuse-tree", args.reuse_tree),
                                          ("--eval-cache", args.eval_cache is not None)) if value]
        if given:
            parser.error(f"{', '.join(given)}: only with --search puct")
    elif args.unique_leaves:
        parser.error("--unique-leaves: only with --search gumbel")
    return args


def puct_setups(args, net_a, net_b):
    """The two EngineSetups of --search puct: A (black in the first leg) searches with --visits / --batch-size, B with
    --white-visits / --white-batch-size where given."""
    from tamago_amd.selfplay.puct_match import EngineSetup
    batch = args.batch_size if args.batch_size is not None else 16
    strict = True if getattr(args, "strict_visits", None) is None else bool(args.strict_visits)
    white_strict = strict if getattr(args, "white_strict_visits", None) is None else bool(args.white_strict_visits)
    return (EngineSetup(net_a, args.visits, batch, strict),
            EngineSetup(net_b, args.white_visits if args.white_visits is not None else args.visits,
                        args.white_batch_size if args.white_batch_size is not None else batch, white_strict))


def main(argv=None):
    args = parse_args(argv)
    from tamago_amd.nn.utility import load_network
    net_a = load_network(args.black, True, args.size)
    net_b = load_network(args.white, True, args.size)
    names = (os.path.basename(args.black), os.path.basename(args.white))
    if args.search == "puct":
        from tamago_amd.selfplay.puct_match import puct_match
        setup_a, setup_b = puct_setups(args, net_a, net_b)
        out = puct_match(setup_a, setup_b, args.games, size=args.size, komi=args.komi, boards=args.boards, swap=args.swap,
                         cgos_mode=args.cgos_mode, check_superko=args.superko, save_dir=args.save_dir, names=names,
                         poll_every=args.poll_every, **(dict(compact_idle=True) if args.compact_idle else {}),
                         **(dict(reuse_tree=True) if args.reuse_tree else {}),
                         **(dict(eval_cache=args.eval_cache) if args.eval_cache else {}))
    else:
        out = search_match(net_a, net_b, args.games, size=args.size, visits=args.visits, komi=args.komi, boards=args.boards,
                           swap=args.swap, save_dir=args.save_dir, names=names, unique_leaves=args.unique_leaves)
    out.pop("results")                                      # (the records are in --save-dir)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
