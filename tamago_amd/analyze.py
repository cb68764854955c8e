"""``python -m tamago_amd.analyze GAME.sgf [GAME.sgf ...]`` - analyse every position of game records, one search tree per
position, many trees at once (tamago_amd/mcts/analysis.py).

Each record is replayed like GTP ``loadsgf`` on a board of its own SZ and KM; the position before every move and the final
position are searched with STRICT ``--visits`` PUCT descents in mini-batches of ``--batch-size`` (``--strict-visits false``:
with the GTP engine's default search, which stops once the runner-up move cannot catch up).  Position k of a game
(k = 0 before the first move) gets the seed ``--seed`` + k, so one game's output does not depend on the other files given.
Games of several sizes are analysed per size.  ``--model`` and the boolean options are read as by ``python -m
tamago_amd.gtp``.

Output on stdout, one line per position, games in the order given:
- ``--format jsonl`` (default): {"game", "move_number" (1-based number of the move played there; n + 1 for the final
  position), "color" (B / W to move), "best" (GTP; pass / resign), "visits" and "winrate" (the root's, as the cgos line),
  "played", "played_visits", "played_winrate", "played_rank" (the move of the record played there: its root child's
  visits, winrate and order among the visited children - 0, null, null if unvisited; all null for the final position),
  "moves" (the cgos-analyze moves list: move, visits, winrate, prior, lcb, order, pv)}.
- ``--format lz``: the GTP lz-analyze ``info ...`` line of each position.

``--sgf-out DIR`` writes DIR/<name of the record> with the record's moves, each with the comment

    B to move, winrate 54.2%, best D5 (321 visits), played C4 (120 visits, winrate 51.0%), top: D5 321 55.1%, C4 120 51.0%, E3 80 49.7%

about the position in which the move was played: the side to move, the root winrate, the most visited move with its visits,
the played move's visits and winrate ("-" for a move without visits), and the three most visited moves with their visits
and winrates (percentages with one decimal).
"""
import argparse
import json
import os
import sys
from collections import OrderedDict

from tamago_amd.gtp.__main__ import _bool, _at_least_one


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m tamago_amd.analyze", description=__doc__.split("\n")[0])
    p.add_argument("games", nargs="+", help="SGF game records")
    p.add_argument("--model", default=os.path.join("model", "model.bin"),
                   help="network parameters (a state_dict saved by torch.save); a file that cannot be loaded leaves the "
                        "network randomly initialised, as in the reference")
    p.add_argument("--visits", type=_at_least_one, default=1000)
    p.add_argument("--batch-size", type=_at_least_one, default=16)
    p.add_argument("--trees", type=_at_least_one, default=None,
                   help="trees searched at once (default: as many as the node-pool memory budget allows)")
    p.add_argument("--superko", type=_bool, default=False)
    p.add_argument("--cgos-mode", type=_bool, default=False)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--pv-depth", type=_at_least_one, default=32)
    p.add_argument("--format", choices=("jsonl", "lz"), default="jsonl")
    p.add_argument("--sgf-out", default=None, help="directory for the annotated copies of the records")
    p.add_argument("--strict-visits", type=_bool, default=True,
                   help="true (default): every position gets exactly --visits descents; false: a position's search stops "
                        "once its runner-up move cannot catch up, as the GTP engine's --visits searches do")
    p.add_argument("--compact-idle", action="store_true",
                   help="leave trees that do not search (decided or pass-only positions, spare trees) out of the forward passes; "
                        "same output")
    p.add_argument("--eval-cache", type=_at_least_one, default=None, metavar="N",
                   help="an evaluation cache of N entries serves positions that were evaluated before (the plies of a record "
                        "overlap); same output")
    p.add_argument("--device-roots", action="store_true",
                   help="set the positions up on the device from the records (no host replay per position); same output")
    return p


def load_games(paths, superko: bool, device_roots: bool = False):
    """(records, positions) per path: {path: (SGFReader, [GamePosition])}; refuses sizes other than 9, 13 and 19.
    device_roots: the positions carry no replayed board (game_record_positions)."""
    from tamago_amd.mcts.analysis import game_positions, game_record_positions
    from tamago_amd.sgf.reader import SGFReader
    games = OrderedDict()
    for path in paths:
        sgf = SGFReader(path, 9)
        games[path] = (sgf, game_record_positions(sgf, path)[1] if device_roots else game_positions(sgf, superko, path))
    return games


def run(args, out=None, network_for=None, games=None):
    """Analyse args.games and write the output (default stdout); network_for(size) -> network (default: load --model).
    Returns {path: [GameAnalysis]}."""
    from tamago_amd.mcts.analysis import GameAnalysis, analyze_positions, annotated_sgf, game_record_positions, game_seeds
    from tamago_amd.mcts.time_manager import TimeControl
    out = out or sys.stdout
    mode = TimeControl.STRICT_PLAYOUT if getattr(args, "strict_visits", True) else TimeControl.CONSTANT_PLAYOUT
    device_roots = bool(getattr(args, "device_roots", False))
    games = games if games is not None else load_games(args.games, args.superko, device_roots)
    if network_for is None:
        from tamago_amd.nn.utility import load_network
        network_for = lambda size: load_network(args.model, True, size)        # noqa: E731
    by_size = OrderedDict()
    for path, (sgf, positions) in games.items():
        by_size.setdefault(sgf.board_size, []).append(path)
    analyses = {}
    for size, paths in by_size.items():
        todo = [(path, p) for path in paths for p in games[path][1]]
        seeds = [s for path in paths for s in game_seeds(args.seed, len(games[path][1]))]
        if device_roots:        # position k of a game is ply k of its record: the roots are written on the device from the records
            where = dict(records=[game_record_positions(games[path][0], path)[0] for path in paths], board_size=size)
            positions = [(g, k) for g, path in enumerate(paths) for k in range(len(games[path][1]))]
        else:
            where = {}
            positions = [(p.board, p.color) for _, p in todo]
        results = analyze_positions(network_for(size), positions, args.visits,
                                    batch_size=args.batch_size, max_trees=args.trees, cgos_mode=args.cgos_mode,
                                    check_superko=args.superko, seeds=seeds, pv_depth=args.pv_depth, mode=mode,
                                    **(dict(compact_idle=True) if getattr(args, "compact_idle", False) else {}),
                                    **(dict(eval_cache=args.eval_cache) if getattr(args, "eval_cache", None) else {}), **where)
        for (path, p), a in zip(todo, results):
            analyses.setdefault(path, []).append(GameAnalysis(p, a))
    for path in games:
        for g in analyses[path]:
            out.write(g.analysis.lz() if args.format == "lz" else json.dumps(g.record()) + "\n")
    if args.sgf_out:
        os.makedirs(args.sgf_out, exist_ok=True)
        for path, (sgf, _) in games.items():
            with open(os.path.join(args.sgf_out, os.path.basename(path)), "w") as f:
                f.write(annotated_sgf(analyses[path], sgf))
    out.flush()
    return analyses


def main(argv=None):
    args = parser().parse_args(argv)
    try:
        games = load_games(args.games, args.superko, args.device_roots)
    except (OSError, ValueError) as exc:
        sys.stderr.write(f"{exc}\n")
        sys.exit(2)
    run(args, games=games)


if __name__ == "__main__":
    main()
