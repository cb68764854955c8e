"""Reanalysis (tamago_amd.mcts.reanalyse.reanalyse_positions) against the per-position loop over
MCTSTree.generate_move_with_sequential_halving, on one GPU.

    python tools/bench_reanalyse.py [--quick] [--out profiles/reanalyse_bench.json]

Records: seeded random play-outs, 8 sampled plies per game as the RL data generator samples them; network: a randomly
initialised DualNet on the device forward.  Rows:
- 9x9, 16 and 100 simulations, 4 096 sampled positions, max_trees 256 and 2 048: positions/s end to end (host replay of
  the boards included) after a warm-up run, and the split into host board replay / root set-up / search / read-out
  (host wall time, the device drained at each boundary), positions forwarded, f16 range fallbacks;
- each of those rows again with "device_roots": true - the same positions in the same process through reanalyse_records
  (the roots written on the device from the records: no host board replay), the yardstick being the row above it;
- the same settings through the per-position loop (the global generator seeded per position, one MCTSTree,
  generate_move_with_sequential_halving, get_root, calculate_improved_policy on the host) over 256 of the same positions;
- 19x19, 16 simulations, 512 positions, max_trees 512, and the loop over 64 of them.
Writes one JSON document (with build.source_digest()) and prints it."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def records(size, games, seed=0):
    """data_generator._Record objects of seeded random play-outs (legal moves, no passes), 8 sampled plies each."""
    import numpy as np
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.nn.data_generator import _Record
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(games):
        board, color, moves = GoBoard(size), 1, []
        for _ in range(rs.randint(size * 2, size * 5)):
            for _ in range(32):
                pos = board.onboard_pos[rs.randint(size * size)]
                if board.cells[pos] == 0 and board.is_legal(pos, color):
                    break
            else:
                break
            board.put_stone(int(pos), color)
            moves.append(int(pos))
            color = 3 - color
        ply = np.sort(rs.permutation(len(moves))[:8])
        out.append(_Record(np.array(moves, dtype=np.int32), ply, rs.permutation(8)[:len(ply)], 1, [""] * len(ply)))
    return out


def network(size):
    import torch
    from oracle.net import make_state_dict
    from tamago_amd.nn.network.dual_net import DualNet
    net = DualNet(torch.device("cuda:0"), size)
    net.load_state_dict(make_state_dict(size, 11, 1.4))
    return net


def lock_step(net, recs, size, visits, trees):
    import torch
    from tamago_amd.mcts.reanalyse import reanalyse_positions
    from tamago_amd.nn.data_generator import _sampled_positions
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pos = list(_sampled_positions(recs, size))
    t1 = time.perf_counter()
    res = reanalyse_positions(net, pos, visits, max_trees=trees)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return {"size": size, "visits": visits, "max_trees": trees, "positions": len(pos),
            "positions_per_s": round(len(pos) / (t2 - t0), 1),
            "seconds": {"board_replay": round(t1 - t0, 3), "root_setup": round(res.seconds["setup"], 3),
                        "search": round(res.seconds["search"], 3), "readout": round(res.seconds["readout"], 3),
                        "total": round(t2 - t0, 3)},
            "forward_positions": res.forward_positions, "range_fallbacks": res.range_fallbacks}, pos


def device_roots(net, recs, size, visits, trees):
    """The lock_step row with the roots written on the device from the records (reanalyse_records): no board replay."""
    import torch
    from tamago_amd.mcts.reanalyse import reanalyse_records
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    members = [(g, int(ply)) for g, r in enumerate(recs) for ply in r.ply]
    t1 = time.perf_counter()
    res = reanalyse_records(net, [r.moves for r in recs], members, visits, max_trees=trees)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return {"size": size, "visits": visits, "max_trees": trees, "positions": len(members), "device_roots": True,
            "positions_per_s": round(len(members) / (t2 - t0), 1),
            "seconds": {"board_replay": round(t1 - t0, 3), "root_setup": round(res.seconds["setup"], 3),
                        "search": round(res.seconds["search"], 3), "readout": round(res.seconds["readout"], 3),
                        "total": round(t2 - t0, 3)},
            "forward_positions": res.forward_positions, "range_fallbacks": res.range_fallbacks, "host_roots": res.host_roots}


def single_loop(net, pos, size, visits):
    import numpy as np
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    tree = MCTSTree(net, tree_size=visits + 16)
    t0 = time.perf_counter()
    for k, (board, color) in enumerate(pos):
        np.random.set_state(np.random.RandomState(k).get_state())
        tree.generate_move_with_sequential_halving(board, color, TimeManager(TimeControl.STRICT_PLAYOUT, visits), True)
        tree.get_root().calculate_improved_policy()
    return {"size": size, "visits": visits, "loop_positions": len(pos),
            "single_tree_loop_positions_per_s": round(len(pos) / (time.perf_counter() - t0), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="512 positions, 64 in the loop, no 19x19 rows (a smoke run of the tool)")
    ap.add_argument("--out", default=os.path.join("profiles", "reanalyse_bench.json"))
    args = ap.parse_args()
    from tamago_amd import build
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    net9 = network(9)
    recs = records(9, 64 if args.quick else 512)
    loop_n = 64 if args.quick else 256
    for visits in (16, 100):
        lock_step(net9, recs[:8], 9, visits, 64)                            # warm-up
        device_roots(net9, recs[:8], 9, visits, 64)
        for trees in (256, 2048):
            row, pos = lock_step(net9, recs, 9, visits, trees)
            emit(row)
            emit(device_roots(net9, recs, 9, visits, trees))                # the same positions, the same process
        single_loop(net9, pos[:4], 9, visits)                               # warm-up
        emit(single_loop(net9, pos[:loop_n], 9, visits))
    if not args.quick:
        net19 = network(19)
        recs19 = records(19, 64, 1)
        lock_step(net19, recs19[:2], 19, 16, 16)                            # warm-up
        row, pos = lock_step(net19, recs19, 19, 16, 512)
        emit(row)
        device_roots(net19, recs19[:2], 19, 16, 16)
        emit(device_roots(net19, recs19, 19, 16, 512))
        single_loop(net19, pos[:2], 19, 16)
        emit(single_loop(net19, pos[:64], 19, 16))
    doc = {"source_digest": build.source_digest(), "command": "python tools/bench_reanalyse.py" + (" --quick" if args.quick else ""),
           "rows": rows}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
