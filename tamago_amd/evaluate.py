"""python -m tamago_amd.evaluate --model MODEL --kifu-dir DIR --size N [--stride K] [--superko] [--json]

How well a network predicts the moves and results of the game records in DIR, and how much of its policy lies outside the
candidates the tree expands (tamago_amd/nn/evaluate.py): a table of ply buckets, or the report as JSON."""
import argparse
import json
import sys


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m tamago_amd.evaluate", description=__doc__.split("\n\n", 1)[1])
    p.add_argument("--model", required=True, help="state_dict of a DualNet (rl-model.bin, sl-model.bin)")
    p.add_argument("--kifu-dir", required=True, help="directory of *.sgf game records")
    p.add_argument("--size", type=int, required=True, choices=(9, 13, 19), help="board size")
    p.add_argument("--stride", type=int, default=1, help="every STRIDE-th ply is evaluated (default 1)")
    p.add_argument("--first-ply", type=int, default=0, help="the first ply evaluated (default 0)")
    p.add_argument("--bucket-width", type=int, default=10, help="plies per bucket (default 10)")
    p.add_argument("--buckets", type=int, default=32, help="buckets; the last takes every later ply (default 32)")
    p.add_argument("--superko", action="store_true", help="candidates under positional superko")
    p.add_argument("--chunk-rows", type=int, default=65536, help="positions per device chunk (default 65536)")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--json", action="store_true", help="print the report as one JSON object")
    return p


def main(argv=None, out=sys.stdout) -> dict:
    args = parser().parse_args(argv)
    from tamago_amd.nn.evaluate import evaluate_records, format_report
    from tamago_amd.nn.utility import load_network
    network = load_network(args.model, True, args.size, args.device)
    report = evaluate_records(network, args.kifu_dir, args.size, stride=args.stride, first_ply=args.first_ply,
                              bucket_width=args.bucket_width, n_buckets=args.buckets, superko=args.superko,
                              chunk_rows=args.chunk_rows, device=args.device)
    print(json.dumps(report) if args.json else format_report(report), file=out)
    return report


if __name__ == "__main__":
    main()
