"""CPU checks of the round-robin tournament (tamago_amd/selfplay/tournament.py): the schedule, the Bradley-Terry fit,
the driver on a fake engine that plays one oracle tree per slot and, like a launch, searches every slot that is not halted -
every game against tests/_puct_match_cases.oracle_puct_game, on 1, 2 and 4 slots -, the argument errors and the command line."""
import json

import numpy as np
import pytest

from tests import _puct_match_cases as pc
from tests._match_cases import make_net
from tests.test_puct_match_host import FakeEngine

SPECS = (("stub", 301), ("stub", 302), ("stub", 303))
NAMES = ("s301", "s302", "s303")
SEARCH = (26, 8)


# ---- the schedule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, rounds", [(2, 1), (3, 1), (3, 2), (5, 3), (64, 1)])
def test_the_schedule_plays_every_ordered_pair(n, rounds):
    from tamago_amd.selfplay.tournament import game_seed, schedule
    pairs = schedule(n, rounds)
    assert len(pairs) == rounds * n * (n - 1)
    once = [(i, j) for i in range(n) for j in range(n) if i != j]
    assert once == sorted(once)                                            # lexicographic
    for r in range(rounds):
        assert pairs[r * len(once):(r + 1) * len(once)] == once
    assert [game_seed(7, k) for k in range(3)] == [7, 8, 9] and game_seed(2 ** 32 - 1, 2) == 1
    for bad in ((1, 1), (3, 0)):
        with pytest.raises(ValueError):
            schedule(*bad)


# ---- the Elo fit ----------------------------------------------------------------------------------------------------------
def test_two_entrants_rate_as_match_rating_does():
    from tamago_amd.selfplay.match import rating
    from tamago_amd.selfplay.tournament import bradley_terry_elo, crosstable_of, pooled_wins
    # A as black: 5 wins, 2 losses, 1 draw; A as white: 3 wins (B as black loses 3), 4 losses, 2 draws; one unfinished
    finished = [(0, 1, "black")] * 5 + [(0, 1, "white")] * 2 + [(0, 1, "draw")] + [(1, 0, "white")] * 3 + [(1, 0, "black")] * 4 + \
               [(1, 0, "draw")] * 2 + [(1, 0, None)]
    table = crosstable_of(2, finished)
    assert table[0][1] == {"wins": 5, "losses": 2, "draws": 1, "unfinished": 0}
    assert table[1][0] == {"wins": 4, "losses": 3, "draws": 2, "unfinished": 1} and table[0][0] is None
    elo = bradley_terry_elo(pooled_wins(table))
    want = rating(8, 6, 3)["elo"]
    assert abs((elo[0] - elo[1]) - want) < 1e-9 and abs(elo[0] + elo[1]) < 1e-9


def test_three_entrants_on_exact_expected_counts():
    """A crosstable of the exact expected (fractional) counts under strengths 0 / +100 / -150 with unequal numbers of games per
    pair: the likelihood equations hold at those strengths, so the fit returns them (mean 0) to 1e-6 Elo."""
    from tamago_amd.selfplay.tournament import bradley_terry_elo
    strength = np.array([0.0, 100.0, -150.0])
    games = np.array([[0, 40, 24], [40, 0, 10], [24, 10, 0]], dtype=np.float64)
    p = 10.0 ** (strength / 400.0)
    wins = games * p[:, None] / (p[:, None] + p[None, :])
    np.fill_diagonal(wins, 0.0)
    elo = bradley_terry_elo(wins)
    assert np.max(np.abs(np.array(elo) - (strength - strength.mean()))) < 1e-6


def test_an_all_win_entrant_is_left_out_and_the_others_are_rated():
    from tamago_amd.selfplay.match import rating
    from tamago_amd.selfplay.tournament import bradley_terry_elo
    wins = [[0, 3, 5, 0], [2, 0, 4, 0], [1, 2, 0, 0], [6, 6, 6, 0]]       # entrant 3 never lost
    elo = bradley_terry_elo(wins)
    assert elo[3] is None and all(e is not None for e in elo[:3]) and abs(sum(elo[:3])) < 1e-9
    assert elo == bradley_terry_elo(wins)                                  # (a pure function)
    assert bradley_terry_elo([r[:3] for r in wins[:3]]) == pytest.approx(elo[:3], abs=1e-9)
    # an all-loss entrant likewise; leaving it out leaves two, rated as a match
    two = bradley_terry_elo([[0, 3, 4], [1, 0, 4], [0, 0, 0]])
    assert two[2] is None and abs((two[0] - two[1]) - rating(3, 1, 0)["elo"]) < 1e-9
    assert bradley_terry_elo([[0, 2], [0, 0]]) == [None, None]


# ---- the driver on a fake engine ------------------------------------------------------------------------------------------
class GroupFake(FakeEngine):
    """FakeEngine with the grouped calls: tree t's network is evaluators[groups[t]], halted slots take no part, every other
    slot searches - a one-child root too."""

    def __init__(self, table):
        super().__init__(table)
        self.forward_positions = 0
        self.forward_positions_by_group = {}
        self.halted = np.ones(self.T, dtype=bool)
        self.groups = np.zeros(self.T, dtype=np.int64)

    def _count(self, n):
        for t in np.flatnonzero(~self.halted):
            g = int(self.groups[t])
            self.forward_positions_by_group[g] = self.forward_positions_by_group.get(g, 0) + n
            self.forward_positions += n

    def root_eval_groups(self, evaluators, groups, halt=None, use_logit=False):
        self.halted = np.zeros(self.T, dtype=bool) if halt is None else np.asarray(halt, dtype=bool).copy()
        self.groups = np.asarray(groups).copy()
        self.log.append(("call", tuple(int(g) if not h else -1 for g, h in zip(self.groups, self.halted))))
        for t in np.flatnonzero(~self.halted):
            self.trees[t].network = evaluators[int(groups[t])]
            self._with_stream(t, lambda: self.trees[t]._initialize_search(self.boards[t], self.colors[t]))
            self.root_children[t] = self.trees[t].node[0].num_children
        self._count(1)

    def puct_chain_groups(self, batches, evaluators):
        def descend(t, leaves):
            tree, scratch = self.trees[t], self.boards[t].clone()
            tree.batch_size = leaves
            for _ in range(leaves):
                scratch.copy_from(self.boards[t])
                tree.search_mcts(scratch, self.colors[t], 0, [])
            assert len(tree.batch_queue.node_index) == 0

        for leaves in batches:
            self.log.append(("batch", leaves))
            for t in np.flatnonzero(~self.halted):                # EVERY tree that is not halted searches
                self._with_stream(t, lambda: descend(t, leaves))
            self._count(leaves)
        return len(batches)


def _entrants():
    return [(name, make_net(spec)) for name, spec in zip(NAMES, SPECS)]


@pytest.fixture(scope="module")
def oracle_games():
    from tamago_amd.selfplay.tournament import schedule
    return [pc.oracle_puct_game(index, SPECS[b], SPECS[w], black_search=SEARCH, white_search=SEARCH, names=(NAMES[b], NAMES[w]))
            for index, (b, w) in enumerate(schedule(3, 1))]


@pytest.fixture(scope="module")
def fake_runs(tmp_path_factory):
    from tamago_amd.selfplay.tournament import puct_tournament
    runs = {}
    for boards in (1, 2, 4):
        engines = []
        save_dir = tmp_path_factory.mktemp(f"tournament{boards}")
        out = puct_tournament(_entrants(), *SEARCH, boards=boards, save_dir=str(save_dir),
                              _make_engine=lambda table: engines.append(GroupFake(table)) or engines[-1])
        runs[boards] = (out, engines[0], save_dir)
    return runs


@pytest.mark.parametrize("boards", [1, 2, 4])
def test_the_driver_plays_the_oracle_games_in_one_engine(fake_runs, oracle_games, boards):
    from tamago_amd.selfplay.tournament import schedule
    out, engine, save_dir = fake_runs[boards]
    pairs = schedule(3, 1)
    assert out["entrants"] == list(NAMES) and out["games"] == 6 and engine.closed
    for i, (text, end, state) in enumerate(oracle_games):
        assert open(save_dir / f"{i}.sgf", encoding="utf-8").read() == text, i
        result = out["results"][i]
        want = pc.oracle_result(text, *end)
        assert {k: result[k] for k in ("winner", "is_resign", "moves")} == {k: want[k] for k in ("winner", "is_resign", "moves")}, i
        assert pc.same_stream(result["stream"], state), i
        assert (result["index"], result["seed"], result["black"], result["white"]) == (i, i, NAMES[pairs[i][0]], NAMES[pairs[i][1]])
    # the crosstable sums to the games, cell by cell
    for i in range(3):
        for j in range(3):
            cell = out["crosstable"][i][j]
            assert (cell is None) == (i == j)
            if cell is not None:
                assert sum(cell.values()) == 1
    assert sum(row["games"] for row in out["standings"]) == 2 * 6 and all(row["games"] == 4 for row in out["standings"])
    assert json.load(open(save_dir / "crosstable.json"))["crosstable"] == out["crosstable"]
    assert len(out["elo"]) == 3
    # every live slot moves in every call: no parking.  A game takes one call per move, and one more where it ends by resignation
    per_game = [end[0] + (1 if end[1] == "resign" else 0) for _, end, _ in oracle_games]
    assert out["moves"] == sum(end[0] for _, end, _ in oracle_games)
    if boards == 1:
        assert out["calls"] == sum(per_game) and out["restarts"] == 5
    else:
        assert max(per_game) <= out["calls"] < sum(per_game)
    calls = [e[1] for e in engine.log if e[0] == "call"]
    assert len(calls) == out["calls"] and all(any(g >= 0 for g in c) for c in calls)
    assert sum(out["forward_positions_by_entrant"]) == out["forward_positions"]
    # what was launched: the roots and descents of the live games, and the descents of one-child roots that searched along
    assert out["leaf_evals"] <= out["forward_positions"] <= out["leaf_evals"] + out["one_child_roots"] * SEARCH[0]
    assert out["leaf_evals"] == out["moves"] + sum(1 for _, end, _ in oracle_games if end[1] == "resign") + \
        (out["moves"] + sum(1 for _, end, _ in oracle_games if end[1] == "resign") - out["one_child_roots"]) * SEARCH[0]


def test_the_three_runs_agree_and_the_groups_change_under_way(fake_runs):
    outs = [fake_runs[b][0] for b in (1, 2, 4)]
    for key in ("crosstable", "standings", "elo", "moves", "leaf_evals", "one_child_roots"):
        assert outs[0][key] == outs[1][key] == outs[2][key], key
    for a, b in zip(outs[0]["results"], outs[2]["results"]):
        assert {k: v for k, v in a.items() if k != "stream"} == {k: v for k, v in b.items() if k != "stream"}
        assert np.array_equal(a["stream"][0], b["stream"][0]) and a["stream"][1] == b["stream"][1]
    # with 4 slots a freed slot restarts in the middle of the run, both colours move in one call and the group sizes change
    engine = fake_runs[4][1]
    calls = [e[1] for e in engine.log if e[0] == "call"]
    sizes = {tuple(sum(1 for g in c if g == k) for k in range(3)) for c in calls}
    assert len(sizes) > 2 and fake_runs[4][0]["restarts"] == 2
    starts = [i for i, e in enumerate(engine.log) if e[0] == "start"]
    assert len(starts) == 6 and all(engine.log[i + 1][0] in ("start", "call") for i in starts)
    assert any(len({g for g in c if g >= 0}) == 3 for c in calls)           # three networks in one launch


def test_argument_errors():
    from tamago_amd.selfplay.puct_match import EngineSetup
    from tamago_amd.selfplay.tournament import puct_tournament
    two = [("a", object()), ("b", object())]
    with pytest.raises(ValueError, match="entrants"):
        puct_tournament(two[:1], 8, 4)
    with pytest.raises(ValueError, match="entrants"):
        puct_tournament([(str(i), object()) for i in range(65)], 8, 4)
    with pytest.raises(ValueError, match="distinct"):
        puct_tournament([("a", object()), ("a", object())], 8, 4)
    with pytest.raises(ValueError, match="name, network"):
        puct_tournament([object(), object()], 8, 4)
    with pytest.raises(ValueError, match="per entrant"):
        puct_tournament([EngineSetup(object(), 8, 4), EngineSetup(object(), 8, 4)], 8, 4)
    with pytest.raises(ValueError, match="at least 1"):
        puct_tournament(two, 0, 4)
    with pytest.raises(ValueError, match="at least 1"):
        puct_tournament(two, 8, 0)
    with pytest.raises(ValueError, match="games_per_pair"):
        puct_tournament(two, 8, 4, games_per_pair=0)
    with pytest.raises(ValueError, match="board size"):
        puct_tournament(two, 8, 4, size=11)
    with pytest.raises(ValueError, match="boards"):
        puct_tournament(two, 8, 4, boards=0)
    with pytest.raises(ValueError, match="seed_base"):
        puct_tournament(two, 8, 4, seed_base=-1)
    with pytest.raises(ValueError, match="resign_threshold"):
        puct_tournament(two, 8, 4, resign_threshold=1.5)
    for option in (dict(reuse_tree=True), dict(eval_cache=1024), dict(strict=False), dict(search="gumbel")):
        with pytest.raises(ValueError, match="not built"):
            puct_tournament(two, 8, 4, **option)

    class Sized:
        board_size = 13

    with pytest.raises(ValueError, match="13x13"):
        puct_tournament([("a", Sized()), ("b", object())], 8, 4, size=9)


def test_the_command_line_reaches_the_driver(monkeypatch, capsys):
    import tamago_amd.nn.utility as utility
    import tamago_amd.selfplay.tournament as tournament
    import tamago_amd.tournament as entry
    assert entry.main is tournament.main
    args = tournament.parse_args(["--models", "a.bin", "b.bin", "--visits", "50"])
    assert (args.names, args.size, args.visits, args.batch_size, args.games_per_pair, args.boards, args.komi, args.seed_base,
            args.save_dir, args.device) == (None, 9, 50, 16, 1, None, 7.0, 0, None, 0)
    for bad in (["--models", "a.bin", "--visits", "8"], ["--models", "a.bin", "b.bin"],
                ["--models", "a.bin", "b.bin", "--visits", "8", "--names", "A"]):
        with pytest.raises(SystemExit):
            tournament.parse_args(bad)
    seen = {}

    def fake(entrants, visits, batch_size, **kwargs):
        seen.update(entrants=entrants, visits=visits, batch_size=batch_size, **kwargs)
        return {"entrants": [n for n, _ in entrants], "results": ["dropped"], "games": 6}

    monkeypatch.setattr(utility, "load_network", lambda path, *a, **k: ("net", path, a))
    monkeypatch.setattr(tournament, "puct_tournament", fake)
    tournament.main(["--models", "x/a.bin", "x/b.bin", "x/c.bin", "--names", "A", "B", "C", "--size", "13", "--visits", "400",
                     "--batch-size", "32", "--games-per-pair", "2", "--boards", "12", "--komi", "6.5", "--seed-base", "100",
                     "--save-dir", "out", "--device", "1"])
    assert seen["entrants"] == [("A", ("net", "x/a.bin", (True, 13))), ("B", ("net", "x/b.bin", (True, 13))),
                                ("C", ("net", "x/c.bin", (True, 13)))]
    assert {k: v for k, v in seen.items() if k != "entrants"} == dict(
        visits=400, batch_size=32, games_per_pair=2, size=13, komi=6.5, boards=12, seed_base=100, save_dir="out", device_index=1)
    assert json.loads(capsys.readouterr().out) == {"entrants": ["A", "B", "C"], "games": 6}
    tournament.main(["--models", "x/a.bin", "y/b.bin", "--visits", "8"])
    assert [n for n, _ in seen["entrants"]] == ["a.bin", "b.bin"]
