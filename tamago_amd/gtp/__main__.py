"""``python -m tamago_amd.gtp`` - the GTP engine program (the reference's main.py:15-95) for GoGui, Sabaki, CGOS ...

Takes the reference's options that this package supports, with the same names, defaults and time-control precedence
(--time over --const-time over --strict-visits over --visits).  The network is always evaluated on the GPU: --use-gpu
false, --policy-move true and the animation options are refused.  --reuse-tree true keeps the subtree of the position
searched next between searches (off by default, like the reference, which rebuilds its tree every move).
--unique-leaves true (with --sequential-halving true) evaluates each distinct leaf of a halving phase once: same moves."""
import argparse
import os
import sys

MCTS_TREE_SIZE = 1 << 16          # mcts/constant.py
NN_BATCH_SIZE = 1
BOARD_SIZE = 9                    # board/constant.py


def _bool(text: str) -> bool:
    """click.BOOL's spellings."""
    value = text.strip().lower()
    if value in ("1", "true", "t", "yes", "y", "on"):
        return True
    if value in ("0", "false", "f", "no", "n", "off"):
        return False
    raise argparse.ArgumentTypeError(f"{text!r} is not a valid boolean")


def _at_least_one(text: str) -> int:
    value = int(text)
    if value < 1:
        raise argparse.ArgumentTypeError(f"{value} is smaller than the minimum valid value 1")
    return value


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m tamago_amd.gtp", description=__doc__.split("\n")[0])
    p.add_argument("--size", type=int, default=BOARD_SIZE, help="board size (9, 13 or 19; default 9)")
    p.add_argument("--superko", type=_bool, default=False)
    p.add_argument("--model", default=os.path.join("model", "model.bin"),
                   help="network parameters (a state_dict saved by torch.save); a file that cannot be loaded leaves the "
                        "network randomly initialised, as in the reference")
    p.add_argument("--use-gpu", type=_bool, default=True)
    p.add_argument("--policy-move", type=_bool, default=False)
    p.add_argument("--sequential-halving", type=_bool, default=False)
    p.add_argument("--komi", type=float, default=7.0)
    p.add_argument("--visits", type=_at_least_one, default=1000)
    p.add_argument("--strict-visits", type=_at_least_one, default=None)
    p.add_argument("--const-time", type=float, default=None)
    p.add_argument("--time", type=float, default=None)
    p.add_argument("--batch-size", type=_at_least_one, default=NN_BATCH_SIZE)
    p.add_argument("--tree-size", type=_at_least_one, default=MCTS_TREE_SIZE)
    p.add_argument("--cgos-mode", type=_bool, default=False)
    p.add_argument("--animation-pv-wait", type=float, default=-1.0)
    p.add_argument("--animation-move-wait", type=float, default=-1.0)
    p.add_argument("--reuse-tree", type=_bool, default=False, nargs="?", const=True,
                   help="keep the searched subtree between moves (default false)")
    p.add_argument("--unique-leaves", type=_bool, default=False, nargs="?", const=True,
                   help="with --sequential-halving true: evaluate each distinct leaf of a phase once (default false)")
    p.add_argument("--device-early-stop", type=_bool, default=False, nargs="?", const=True,
                   help="with --visits: the early-stop test of a search runs on the device, the mini-batches are queued "
                        "without a read-back in between (same moves; default false)")
    p.add_argument("--eval-cache", type=_at_least_one, default=None, metavar="N",
                   help="an evaluation cache of N entries serves positions that were evaluated before - the subtree under the "
                        "move played is searched again a ply later (same moves; default off)")
    return p


def check_options(args) -> str:
    """Why the options cannot be served ('' if they can)."""
    if not args.use_gpu:
        return "--use-gpu false is not supported: this engine evaluates its network on the GPU only"
    if args.policy_move:
        return "--policy-move true is not supported: moves come from the tree search"
    if args.animation_pv_wait >= 0 or args.animation_move_wait >= 0:
        return "--animation-pv-wait / --animation-move-wait are not supported"
    if args.size not in (9, 13, 19):
        return f"--size {args.size} is not supported (9, 13 or 19)"
    return ""


def main(argv=None):
    args = parser().parse_args(argv)
    problem = check_options(args)
    if problem:
        sys.stderr.write(problem + "\n")
        sys.exit(2)
    from tamago_amd.gtp.client import GtpClient
    from tamago_amd.mcts.time_manager import TimeControl
    from tamago_amd.nn.utility import load_network

    mode, visits = TimeControl.CONSTANT_PLAYOUT, args.visits
    if args.strict_visits is not None:
        mode, visits = TimeControl.STRICT_PLAYOUT, args.strict_visits
    if args.const_time is not None:
        mode = TimeControl.CONSTANT_TIME
    if args.time is not None:
        mode = TimeControl.TIME_CONTROL
    network = load_network(args.model, True, args.size)
    client = GtpClient(args.size, args.superko, network, komi=args.komi, mode=mode, visits=visits,
                       const_time=args.const_time if args.const_time is not None else 5.0,
                       time=args.time if args.time is not None else 0.0, batch_size=args.batch_size,
                       tree_size=args.tree_size, cgos_mode=args.cgos_mode,
                       use_sequential_halving=args.sequential_halving, reuse_tree=args.reuse_tree,
                       unique_leaves=args.unique_leaves, device_early_stop=args.device_early_stop,
                       **(dict(eval_cache=args.eval_cache) if args.eval_cache else {}))
    client.run()


if __name__ == "__main__":
    main()
