"""Helper of test_gpu_match.py (also run as a script: the scheme of the one-call move - TG_SP_CHAIN - is read from the
environment per handle, and a test sets it for a child process only).  Two seeded random-init DualNets play a swapped match
through tg_selfplay_play_move2; prints a digest of the records and the tally as one JSON line:
argv = boards, games, visits, unique_leaves (0 / 1)."""
import hashlib
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TALLY_KEYS = ("games", "wins_a", "wins_b", "draws", "unfinished", "as_black", "as_white", "resignations", "mean_length",
              "leaf_evals", "moves", "score_a", "elo", "elo_interval")


def two_nets(size=9):
    import torch
    from tamago_amd.nn.network.dual_net import DualNet
    torch.manual_seed(21)
    net_a = DualNet(torch.device("cuda:0"), size)
    torch.manual_seed(22)
    net_b = DualNet(torch.device("cuda:0"), size)
    return net_a, net_b


def play(net_a, net_b, boards, games, visits, unique_leaves=False):
    """(digest of the 2 * games records, the tally) of games 1..games played from both sides."""
    from tamago_amd.selfplay.match import search_match
    h = hashlib.sha256()
    with tempfile.TemporaryDirectory() as d:
        out = search_match(net_a, net_b, games, size=9, visits=visits, boards=boards, swap=True,
                           seeds=list(range(1, games + 1)), save_dir=d, unique_leaves=unique_leaves)
        for i in range(2 * games):
            h.update(open(os.path.join(d, f"{i}.sgf"), "rb").read())
    return h.hexdigest()[:16], {k: out[k] for k in TALLY_KEYS}, out


if __name__ == "__main__":
    boards, games, visits, unique = (int(v) for v in sys.argv[1:5])
    digest, tally, out = play(*two_nets(), boards, games, visits, bool(unique))
    from tamago_amd import lib
    from tamago_amd.selfplay.match import handle_is_chained
    print(json.dumps({"digest": digest, "tally": tally, "range_fallbacks": out["range_fallbacks"],
                      "chained": handle_is_chained(lib.load())}))
