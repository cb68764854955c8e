"""evaluate_records (tamago_amd/nn/evaluate.py) on the golden game records against a host pipeline on the same
network: GoBoard replay, generate_input_planes, tg_net_forward_host on the same rows in the same chunking, and the numpy
restatement of tests/_row_score_cases.py.  Row records and counts are exact while the network reports no range fallback (the
caveat of every comparison between two forward paths here); which plies stride and first_ply select; a record with a bad move
is redone on the host and named; the command line's JSON is the function's report."""
import io
import json

import numpy as np
import pytest

from tests import _eval_cases as ec
from tests import _row_score_cases as cases
from tests._replay_records import random_record, sgf_text

pytestmark = pytest.mark.gpu

CHUNK = {9: 60, 13: 50, 19: 50}             # rows per chunk: more than one chunk, and one of a single game


def _network(size, seed=11):
    import torch
    from tamago_amd.nn.network.dual_net import DualNet, random_state_dict
    torch.manual_seed(seed + size)
    net = DualNet(torch.device("cuda", 0), size)
    net.load_state_dict(random_state_dict(size))
    return net


def _check(report, host, size, n_buckets=32):
    want, row_game, row_ply = host
    assert report["range_fallbacks"] == 0
    assert report["positions"] == len(want) == len(report["rows"])
    assert np.array_equal(report["row_game"], row_game) and np.array_equal(report["row_ply"], row_ply)
    cases.check_records(report["rows"], want)
    cases.check_table(report["table"], want, n_buckets, report["rows"]["cand_mass"])
    counts = cases.restate_table(want, n_buckets)[0].sum(axis=0)
    t = report["totals"]
    assert (t["rows"], t["invalid_rows"]) == (int(counts[0]), int(counts[5]))
    if counts[0] == 0:                                                       # nothing sampled: no rate is defined
        assert t["top1"] is None and t["policy_loss"] is None and t["prior_mass_lost"] is None
        return
    assert t["top1"] == counts[1] / counts[0] and t["top5"] == counts[2] / counts[0]
    assert t["value_hit_rate"] == counts[4] / counts[0] and t["moves_never_expanded"] == counts[3] / counts[0]
    assert 0.0 < t["prior_mass_on_candidates"] <= 1.0 + 1e-6 and abs(t["prior_mass_lost"] - (1.0 - t["prior_mass_on_candidates"])) < 1e-15
    assert sum(b["rows"] for b in report["buckets"]) == t["rows"]


@pytest.mark.parametrize("size,superko", [(9, False), (9, True), (13, False), (19, False)])
def test_report_equals_the_host_pipeline(tmp_path, size, superko):
    from tamago_amd.nn.evaluate import evaluate_records
    net = _network(size)
    paths = ec.write_games(tmp_path / "games", size)
    report = evaluate_records(net, paths, size, superko=superko, chunk_rows=CHUNK[size], rows=True)
    assert report["games"] == len(paths) and report["host_games"] == [] and report["superko"] is superko
    _check(report, ec.host_pipeline(net, paths, size, superko=superko, chunk_rows=CHUNK[size]), size)
    # a directory is its sorted *.sgf; without rows=True the report is plain data
    plain = evaluate_records(net, str(tmp_path / "games"), size, superko=superko, chunk_rows=CHUNK[size])
    assert "rows" not in plain and plain["totals"] == report["totals"] and plain["buckets"] == report["buckets"]
    json.dumps(plain)


def test_stride_and_first_ply_select_the_plies_they_say(tmp_path):
    from tamago_amd.nn import evaluate as ev
    size = 9
    net = _network(size)
    paths = ec.write_games(tmp_path / "games", size)
    lengths = [len(ev.read_record(p, size).moves) for p in paths]
    for stride, first_ply, bw, nb in ((3, 2, 10, 32), (1, 30, 4, 5), (7, 0, 1, 3), (1, 10000, 10, 32)):
        report = ev.evaluate_records(net, paths, size, stride=stride, first_ply=first_ply, bucket_width=bw, n_buckets=nb, rows=True)
        want_ply = [p for n in lengths for p in range(first_ply, n, stride)]
        want_game = [g for g, n in enumerate(lengths) for _ in range(first_ply, n, stride)]
        assert report["row_ply"].tolist() == want_ply and report["row_game"].tolist() == want_game
        assert report["rows"]["bucket"].tolist() == [min(p // bw, nb - 1) for p in want_ply]
        _check(report, ec.host_pipeline(net, paths, size, stride=stride, first_ply=first_ply, bucket_width=bw, n_buckets=nb), size, nb)
        if not want_ply:
            assert report["totals"]["rows"] == 0 and report["totals"]["top1"] is None


def test_a_record_with_a_bad_move_is_redone_on_the_host(tmp_path):
    """A move onto a point that holds a stone: the device replay stops there and flags the game, the host board plays it as
    the data generators do, and every row of the report is the host pipeline's."""
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.nn.evaluate import evaluate_records
    size = 9
    moves = random_record(size, 40, 6)
    board = GoBoard(size)
    for ply, pos in enumerate(moves[:25]):
        board.put_stone(pos, 1 + ply % 2)
    moves[25] = next(p for p in board.onboard_pos if board.cells[p] != 0)
    net = _network(size)
    paths = ec.write_games(tmp_path / "games", size, extra=[("00_bad", sgf_text(size, moves, "W+2.5"))])
    report = evaluate_records(net, paths, size, chunk_rows=CHUNK[size], rows=True)
    assert report["host_games"] == [paths[0]] and paths[0].endswith("00_bad.sgf")
    assert (report["row_game"] == 0).sum() == 40
    _check(report, ec.host_pipeline(net, paths, size, chunk_rows=CHUNK[size]), size)


def test_the_command_line_json_is_the_report(tmp_path):
    import torch
    import tamago_amd.evaluate as cli
    from tamago_amd.nn.evaluate import evaluate_records
    size = 9
    net = _network(size)
    model = str(tmp_path / "model.bin")
    torch.save(net.state_dict(), model)
    paths = ec.write_games(tmp_path / "games", size)
    want = evaluate_records(net, paths, size, stride=2, superko=True)
    out, grad = io.StringIO(), torch.is_grad_enabled()
    try:
        cli.main(["--model", model, "--kifu-dir", str(tmp_path / "games"), "--size", "9", "--stride", "2", "--superko", "--json"], out=out)
    finally:
        torch.set_grad_enabled(grad)                                          # (load_network turns it off, as the reference does)
    assert json.loads(out.getvalue()) == json.loads(json.dumps(want))
    out = io.StringIO()
    try:
        cli.main(["--model", model, "--kifu-dir", str(tmp_path / "games"), "--size", "9"], out=out)
    finally:
        torch.set_grad_enabled(grad)
    assert out.getvalue().splitlines()[0].startswith(f"{len(paths)} games") and " all " in out.getvalue()


def test_behind_an_evaluation_cache(tmp_path):
    """eval_cache=: the forward pass goes through a CachedEvaluator - every row is looked up and none is uncacheable (the
    replay's planes are canonical), and a second evaluation of the same records finds rows in the table."""
    from tamago_amd.nn.eval_cache import EvalCache
    from tamago_amd.nn.evaluate import evaluate_records
    size = 9
    net = _network(size)
    paths = ec.write_games(tmp_path / "games", size)
    cache = EvalCache(size, 65536)
    try:
        first = evaluate_records(net, paths, size, eval_cache=cache)
        stats = cache.stats(reset=True)
        assert stats["lookups"] == first["positions"] and stats["uncacheable"] == 0 and stats["inserts"] > 0
        second = evaluate_records(net, paths, size, eval_cache=cache)
        stats = cache.stats()
        assert stats["lookups"] == second["positions"] == first["positions"] and stats["hits"] > 0
        assert second["totals"]["rows"] == first["totals"]["rows"]
    finally:
        cache.close()
