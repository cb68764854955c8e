"""One or more generations of the reference's pipeline (pipeline.sh: self-play -> train; the
GNU Go adjudication step is out of scope) on one GPU, every stage on this repo's path:

    python tools/rl_loop.py <program_dir> [generations] [games] [boards] [visits] [batch] [unique_leaves 0|1] [gate_games]
                             [device_data 0|1] [reanalyse_visits] [gate_visits] [device_roots 0|1] [gate_search gumbel|puct]
                             [gate_batch] [gate_reuse 0|1] [eval_dir PATH]

  self-play   tamago_amd.selfplay.worker.selfplay_shard   (HIP search + forward, SGF records)
  data        tamago_amd.nn.data_generator                (HIP featurise, rl_data_*.npz; device_data 1: the records are
                                                           replayed on the device, tg_replay_run, and the chunks go to the
                                                           trainer in device memory, without a file)
  reanalyse   tamago_amd.nn.data_generator                (reanalyse_visits > 0, from generation 1 on: the records of the
                                                           generation before are searched again by the network that plays
                                                           this one, iter_reanalysed_chunks with that many simulations, and
                                                           their chunks are trained on after the new ones; the chunks of
                                                           such a generation are made in device memory, as with device_data;
                                                           device_roots 1: the search roots are written on the device from
                                                           the records, without a host replay per position)
  train       tamago_amd.nn.learn                         (fp32 step, rl-model.bin / rl-state.ckpt)
  gate        tamago_amd.policy_games.match               (gate_games > 0: the trained network against the one before
                                                           training, policy against policy, both colours; logged only)
              tamago_amd.selfplay.match.search_match      (gate_games > 0 and gate_visits > 0 instead: the same pairing
                                                           under Gumbel search with gate_visits simulations per move, as
                                                           the networks are deployed; logged with its Elo estimate)
              tamago_amd.selfplay.puct_match.puct_match   (gate_search puct with gate_games > 0 and gate_visits > 0: the
                                                           pairing under the PUCT search the GTP engine plays with,
                                                           gate_visits strict visits per move in mini-batches of
                                                           gate_batch, default 16; gate_reuse 1: with tree
                                                           reuse, one tree per game and colour kept across the moves,
                                                           as the engine plays under --reuse-tree)
  evaluate    tamago_amd.nn.evaluate.evaluate_records     (a trailing `eval_dir PATH` pair: the trained network of every
                                                           generation on the held-out records in PATH - move prediction,
                                                           value, prior mass on the tree's candidates; logged only)
"""
import glob
import os
import sys
import time

ROOT = os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import tamago_amd.nn.data_generator as dg  # noqa: E402
from tamago_amd.nn import learn  # noqa: E402
from tamago_amd.nn.network.dual_net import DualNet  # noqa: E402
from tamago_amd.selfplay.worker import selfplay_shard  # noqa: E402


def run_generation(program_dir, generation, games, boards, visits, batch, size=9, log=print, unique_leaves=False,
                   gate_games=0, device_data=False, reanalyse_visits=0, gate_visits=0, device_roots=False,
                   gate_search="gumbel", gate_batch=16, gate_reuse=False, eval_dir=None):
    if gate_search not in ("gumbel", "puct"):
        raise ValueError(f"gate_search is 'gumbel' or 'puct', not {gate_search!r}")
    device = torch.device("cuda", 0)
    model = os.path.join(program_dir, "model", "rl-model.bin")
    net = DualNet(device, size)
    if os.path.exists(model):
        net.load_state_dict(torch.load(model, map_location="cpu"))
    else:                                   # generation 0 starts from the random initialisation
        os.makedirs(os.path.dirname(model), exist_ok=True)
        torch.save(net.state_dict(), model)
    kifu_dir = os.path.join(program_dir, "archive", str(generation))
    os.makedirs(kifu_dir, exist_ok=True)
    first = generation * games + 1
    t0 = time.time()
    stats = selfplay_shard(kifu_dir, net, list(range(first, first + games)), size, visits, boards=boards,
                           unique_leaves=unique_leaves)
    t1 = time.time()
    for old in glob.glob(os.path.join(program_dir, "data", "rl_data_*.npz")):
        os.remove(old)
    os.makedirs(os.path.join(program_dir, "data"), exist_ok=True)
    previous_dir = os.path.join(program_dir, "archive", str(generation - 1))
    reanalyse = reanalyse_visits > 0 and generation >= 1 and os.path.isdir(previous_dir)
    if device_data or reanalyse:             # (the chunks are made here, so that the stage times mean what they meant)
        chunks = list(dg.iter_reinforcement_learning_chunks([kifu_dir], size, device))
        if reanalyse:                        # (after the new chunks: their random draws are those of a run without it)
            before = dict(dg.REANALYSE_STATS)
            chunks += list(dg.iter_reanalysed_chunks(net, [previous_dir], size, reanalyse_visits, device,
                                                     seed=generation << 24, device_roots=device_roots))
            done = {k: dg.REANALYSE_STATS[k] - before[k] for k in before}
            log(f"generation {generation}: reanalysed {done['positions']} positions of generation {generation - 1} with "
                f"{reanalyse_visits} simulations: boards {done['board_seconds']:.1f} s, search {done['search_seconds']:.1f} s, "
                f"{done['forward_positions']} positions forwarded, {done['range_fallbacks']} range fallbacks")
        torch.cuda.synchronize(device)
    else:
        chunks = None
        dg.generate_reinforcement_learning_data(program_dir, [kifu_dir], size)
    t2 = time.time()
    loss = learn.train_with_gumbel_alphazero_on_gpu(program_dir, size, batch, chunks=chunks)
    t3 = time.time()
    if gate_games > 0 and gate_visits > 0 and gate_search == "puct":
        from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
        new = DualNet(device, size)
        new.load_state_dict(torch.load(model, map_location="cpu"))
        gate = puct_match(EngineSetup(new, gate_visits, gate_batch), EngineSetup(net, gate_visits, gate_batch), gate_games,
                          size=size, swap=True, names=("new", "previous"), **(dict(reuse_tree=True) if gate_reuse else {}))
        elo = "unbounded" if gate["elo"] is None else f"{gate['elo']:+.0f}"
        low, high = ("-inf" if v is None and i == 0 else "+inf" if v is None else f"{v:+.0f}"
                     for i, v in enumerate(gate["elo_interval"]))
        log(f"generation {generation}: new against previous over {gate['games']} PUCT games at {gate_visits} visits in "
            f"mini-batches of {gate_batch}{' with tree reuse' if gate_reuse else ''}: {gate['wins_a']} won, {gate['wins_b']} lost, {gate['draws']} drawn, "
            f"{gate['unfinished']} unfinished, {gate['resignations']} resigned (mean length {gate['mean_length']:.1f}, "
            f"{gate['games_per_second']:.0f} games/s, {gate['leaf_evals']} leaf-evals, {gate['range_fallbacks']} range "
            f"fallbacks); score {gate['score_a']}, Elo {elo} [{low}, {high}]")
    elif gate_games > 0 and gate_visits > 0:
        from tamago_amd.selfplay.match import search_match
        new = DualNet(device, size)
        new.load_state_dict(torch.load(model, map_location="cpu"))
        gate = search_match(new, net, gate_games, size=size, visits=gate_visits, swap=True, names=("new", "previous"))
        elo = "unbounded" if gate["elo"] is None else f"{gate['elo']:+.0f}"
        low, high = ("-inf" if v is None and i == 0 else "+inf" if v is None else f"{v:+.0f}"
                     for i, v in enumerate(gate["elo_interval"]))
        log(f"generation {generation}: new against previous over {gate['games']} search games at {gate_visits} simulations: "
            f"{gate['wins_a']} won, {gate['wins_b']} lost, {gate['draws']} drawn, {gate['unfinished']} unfinished, "
            f"{gate['resignations']} resigned (mean length {gate['mean_length']:.1f}, {gate['games_per_second']:.0f} games/s, "
            f"{gate['leaf_evals']} leaf-evals); score {gate['score_a']}, Elo {elo} [{low}, {high}]")
    elif gate_games > 0:
        from tamago_amd.policy_games import match
        new = DualNet(device, size)
        new.load_state_dict(torch.load(model, map_location="cpu"))
        gate = match(new, net, gate_games, size=size, swap=True)
        log(f"generation {generation}: new against previous over {gate['games']} policy games: {gate['wins_a']} won, "
            f"{gate['wins_b']} lost, {gate['draws']} drawn, {gate['unfinished']} unfinished "
            f"(mean length {gate['mean_length']:.1f}, {gate['games_per_second']:.0f} games/s)")
    if eval_dir:
        from tamago_amd.nn.evaluate import evaluate_records
        new = DualNet(device, size)
        new.load_state_dict(torch.load(model, map_location="cpu"))
        t = evaluate_records(new, eval_dir, size)
        e = t["totals"]
        if e["rows"]:
            log(f"generation {generation}: new on {t['games']} held-out games / {e['rows']} positions: top-1 {e['top1']:.3f}, "
                f"top-5 {e['top5']:.3f}, policy loss {e['policy_loss']:.4f}, value loss {e['value_loss']:.4f}, value hits "
                f"{e['value_hit_rate']:.3f}, Brier {e['brier']:.4f}, prior mass off the candidates {e['prior_mass_lost']:.5f}, "
                f"moves never expanded {e['moves_never_expanded']:.4f} ({e['invalid_rows']} invalid rows, "
                f"{len(t['host_games'])} games redone on the host)")
        else:
            log(f"generation {generation}: no position to evaluate in {eval_dir}")
    log(f"generation {generation}: self-play {stats['games']} games / {stats['leaf_evals']} leaf-evals "
        f"({stats['forward_positions']} positions forwarded) "
        f"in {t1 - t0:.1f} s, data {t2 - t1:.1f} s, train {t3 - t2:.1f} s, last-chunk loss sums {loss}")
    return stats, loss


def split_eval_dir(argv):
    """The trailing `eval_dir PATH` pair off the positional arguments: (the arguments without it, PATH or None)."""
    if "eval_dir" not in argv:
        return list(argv), None
    i = argv.index("eval_dir")
    if i + 2 != len(argv):
        raise SystemExit("eval_dir PATH is the last pair of the command line")
    return list(argv[:i]), argv[i + 1]


if __name__ == "__main__":
    a, eval_dir = split_eval_dir(sys.argv[1:])
    program_dir = a[0]
    gens, games, boards, visits, batch = (int(x) for x in (a[1:6] + ["2", "256", "256", "16", "256"][len(a[:6]) - 1:]))
    unique = len(a) > 6 and a[6].lower() in ("1", "true", "yes")
    gate_games = int(a[7]) if len(a) > 7 else 0
    device_data = len(a) > 8 and a[8].lower() in ("1", "true", "yes")
    reanalyse_visits = int(a[9]) if len(a) > 9 else 0
    gate_visits = int(a[10]) if len(a) > 10 else 0
    device_roots = len(a) > 11 and a[11].lower() in ("1", "true", "yes")
    gate_search = a[12].lower() if len(a) > 12 else "gumbel"
    gate_batch = int(a[13]) if len(a) > 13 else 16
    gate_reuse = len(a) > 14 and a[14].lower() in ("1", "true", "yes")
    dg.BATCH_SIZE = batch
    for g in range(gens):
        run_generation(program_dir, g, games, boards, visits, batch, unique_leaves=unique, gate_games=gate_games,
                       device_data=device_data, reanalyse_visits=reanalyse_visits, gate_visits=gate_visits,
                       device_roots=device_roots, gate_search=gate_search, gate_batch=gate_batch, gate_reuse=gate_reuse,
                       eval_dir=eval_dir)
