"""Policy against policy: whole games on the device, one forward position per ply and board.

    python -m tamago_amd.policy_games --black A.bin --white B.bin --games N [--size 9] [--boards B] [--komi 7.0]
                                      [--swap true] [--superko true] [--max-moves M]

prints one JSON line: wins of A and of B, draws, unfinished games (those that reached the move limit), mean length,
games per second.  With --swap both colour assignments are played (N games each) and added up.  Every move is
nn/policy_player.py's generate_move_from_policy with the engine rule of gtp/client.py:209-211 (a pass is answered with a
pass); game g draws from the stream of random.Random(g).
"""
import argparse
import json
import time


def _flag(text: str) -> bool:
    return text.lower() in ("1", "true", "yes")


def match(net_a, net_b, games: int, size: int = 9, komi: float = 7.0, boards=None, swap: bool = False,
          superko: bool = True, max_moves=None, device_index: int = 0) -> dict:
    """net_a against net_b: `games` games with net_a black and, with swap, `games` more with net_a white."""
    from tamago_amd.nn.policy_player import policy_games
    out = {"games": 0, "wins_a": 0, "wins_b": 0, "draws": 0, "unfinished": 0, "positions": 0}
    lengths = 0
    start = time.time()
    for a_is_black in ((True, False) if swap else (True,)):
        black, white = (net_a, net_b) if a_is_black else (net_b, net_a)
        res = policy_games(black, white, games, size=size, komi=komi, max_moves=max_moves, boards=boards, superko=superko,
                           device_index=device_index)
        for game in res["games"]:
            lengths += game["length"]
            if game["winner"] is None:
                out["unfinished"] += 1
            elif game["winner"] == "draw":
                out["draws"] += 1
            else:
                out["wins_a" if (game["winner"] == "black") == a_is_black else "wins_b"] += 1
        out["games"] += games
        out["positions"] += res["positions"]
    seconds = time.time() - start
    out["mean_length"] = lengths / out["games"]
    out["seconds"] = seconds
    out["games_per_second"] = out["games"] / seconds
    return out


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m tamago_amd.policy_games")
    parser.add_argument("--black", required=True, help="model file of network A (black in the first leg)")
    parser.add_argument("--white", required=True, help="model file of network B")
    parser.add_argument("--games", type=int, required=True)
    parser.add_argument("--size", type=int, default=9)
    parser.add_argument("--boards", type=int, default=None)
    parser.add_argument("--komi", type=float, default=7.0)
    parser.add_argument("--swap", type=_flag, default=False)
    parser.add_argument("--superko", type=_flag, default=True)
    parser.add_argument("--max-moves", type=int, default=None)
    args = parser.parse_args(argv)
    from tamago_amd.nn.utility import load_network
    net_a = load_network(args.black, True, args.size)
    net_b = load_network(args.white, True, args.size)
    print(json.dumps(match(net_a, net_b, args.games, args.size, args.komi, args.boards, args.swap, args.superko,
                           args.max_moves)))


if __name__ == "__main__":
    main()
