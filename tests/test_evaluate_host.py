"""The host side of the evaluation on game records (tamago_amd/nn/evaluate.py, tamago_amd/board/candidates.py) - no GPU: the host
candidate filter, which flagged games are redone with, against the reference-written lists of the rule corpus; the sampling,
chunking and move-index rules; the report from a table; the command line's options and the rl_loop pair."""
import io
import json
import os
import sys

import numpy as np
import pytest

from tests import _eval_cases as ec
from tests import _row_score_cases as cases
from tests import _rule_corpus as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("size", rc.SIZES)
def test_host_candidates_equal_the_reference_lists(size):
    """Every entry of the corpus, the history-limit entries included, superko off and on."""
    fx = rc.load_fixture(size)
    differ = 0
    for i, entry in enumerate(fx.entries):
        for superko in (0, 1):
            assert ec.host_candidates(size, i, superko) == fx.cand[superko][i], (entry.name, superko)
        differ += fx.cand[0][i] != fx.cand[1][i]
    assert differ >= 5


def test_sampling_chunking_and_move_indices():
    from tamago_amd.nn import evaluate as ev
    assert ev.sampled_plies(10, 1, 0).tolist() == list(range(10))
    assert ev.sampled_plies(10, 3, 2).tolist() == [2, 5, 8]
    assert ev.sampled_plies(10, 3, 10).tolist() == [] and ev.sampled_plies(0, 1, 0).tolist() == []
    w = 11
    moves = np.array([0, w + 1, w + 9, 9 * w + 9, 5, w, w + 10, 10 * w + 3, 500, -4], dtype=np.int32)
    assert ev.move_actions(moves, 9).tolist() == [81, 0, 8, 80, -1, -1, -1, -1, -1, -1]
    records = [ev.EvalRecord(np.zeros(n, np.int32), 1) for n in (5, 5, 12, 0, 3, 4)]
    assert list(ev.chunk_games(records, 1, 0, 10)) == [(0, 2), (2, 1), (3, 3)]          # whole games; a game beyond the limit alone
    assert list(ev.chunk_games(records, 1, 0, 1000)) == [(0, 6)]
    assert list(ev.chunk_games(records, 2, 1, 4)) == [(0, 2), (2, 1), (3, 3)]           # 2, 2 | 6 | 0, 1, 2 rows
    assert list(ev.chunk_games([], 1, 0, 10)) == []


def test_report_from_a_table():
    from tamago_amd.nn import evaluate as ev
    assert ev.ROW_DTYPE == cases.ROW_DTYPE and ev.BUCKET_DTYPE == cases.BUCKET_DTYPE
    table = np.zeros(3, dtype=ev.BUCKET_DTYPE)
    table["count"][0] = [4, 1, 3, 1, 2, 0]
    table["sum"][0] = [8.0, 3.0, 2.0, 1.0]
    table["count"][2] = [6, 3, 6, 0, 3, 2]
    table["sum"][2] = [3.0, 6.0, 12.0, 0.75]
    rep = ev.report_from_table(table, 10)
    b0, b1, b2 = rep["buckets"]
    assert (b0["first_ply"], b0["last_ply"], b2["first_ply"], b2["last_ply"]) == (0, 9, 20, None)
    assert b0 == dict(b0, rows=4, top1=0.25, top5=0.75, policy_loss=2.0, value_loss=0.5, value_hit_rate=0.5, brier=0.25,
                      prior_mass_on_candidates=0.75, prior_mass_lost=0.25, moves_never_expanded=0.25, invalid_rows=0)
    assert b1["rows"] == 0 and b1["top1"] is None and b1["prior_mass_lost"] is None
    t = rep["totals"]
    assert (t["rows"], t["invalid_rows"], t["top1"], t["top5"], t["policy_loss"], t["value_hit_rate"]) == (10, 2, 0.4, 0.9, 1.1, 0.5)
    assert t["prior_mass_on_candidates"] == 0.9 and abs(t["prior_mass_lost"] - 0.1) < 1e-15 and t["moves_never_expanded"] == 0.1
    rep.update(board_size=9, games=2, positions=12, stride=1, first_ply=0, superko=False, host_games=[])
    json.dumps(rep)
    text = ev.format_report(rep)
    assert "all" in text and "20-" in text and "10-19" not in text


def test_the_command_line(monkeypatch):
    import tamago_amd.evaluate as cli
    args = cli.parser().parse_args(["--model", "m.bin", "--kifu-dir", "games", "--size", "13"])
    assert (args.stride, args.superko, args.json, args.first_ply, args.bucket_width, args.buckets) == (1, False, False, 0, 10, 32)
    args = cli.parser().parse_args(["--model", "m.bin", "--kifu-dir", "games", "--size", "9", "--stride", "4", "--superko", "--json"])
    assert (args.stride, args.superko, args.json) == (4, True, True)
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["--model", "m.bin", "--kifu-dir", "games", "--size", "11"])
    # the options reach evaluate_records; --json prints the report
    import tamago_amd.nn.evaluate as ev
    import tamago_amd.nn.utility as utility
    seen = {}

    def fake(network, records, size, **kwargs):
        seen.update(kwargs, network=network, records=records, size=size)
        return {"totals": {"rows": 3}, "buckets": []}
    monkeypatch.setattr(ev, "evaluate_records", fake)
    monkeypatch.setattr(utility, "load_network", lambda path, use_gpu, size, device: ("net", path, size))
    out = io.StringIO()
    cli.main(["--model", "m.bin", "--kifu-dir", "games", "--size", "9", "--stride", "4", "--superko", "--json"], out=out)
    assert json.loads(out.getvalue()) == {"totals": {"rows": 3}, "buckets": []}
    assert seen["network"] == ("net", "m.bin", 9) and seen["records"] == "games" and seen["size"] == 9
    assert seen["stride"] == 4 and seen["superko"] is True and seen["n_buckets"] == 32


def test_the_rl_loop_pair():
    """A trailing `eval_dir PATH` pair, off by default; the positional arguments keep their places."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import rl_loop
    finally:
        sys.path.pop(0)
    assert rl_loop.split_eval_dir(["prog", "2", "64"]) == (["prog", "2", "64"], None)
    assert rl_loop.split_eval_dir(["prog", "2", "64", "eval_dir", "held_out"]) == (["prog", "2", "64"], "held_out")
    assert rl_loop.split_eval_dir(["prog", "eval_dir", "held_out"]) == (["prog"], "held_out")
    with pytest.raises(SystemExit):
        rl_loop.split_eval_dir(["prog", "2", "eval_dir"])
    import inspect
    assert inspect.signature(rl_loop.run_generation).parameters["eval_dir"].default is None
