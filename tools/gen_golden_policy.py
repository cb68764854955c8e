#!/usr/bin/env python3
"""Golden moves of the REFERENCE's policy player (nn/policy_player.py:13-46 generate_move_from_policy), called as it
stands with a stub network whose ``inference`` returns a recorded vector, and of its GTP engine mode
(gtp/client.py:206-211, policy_move=True).  The reference is imported at run time from the checkout named by
TAMAGO_REFERENCE (never copied into this repository; for 13x13 / 19x19 a scratch copy with the board-size constant
changed is made in a temporary directory and deleted afterwards, as tools/gen_golden.py does):

    TAMAGO_REFERENCE=<reference checkout> python tools/gen_golden_policy.py

-> tests/golden/policy_moves_s{9,13,19}.npz (policy vectors, float32) + .json (cases, labels, expected results).
A case: the moves to replay (alternating colours from black, padded coordinates, 0 = pass), the superko flag, the colour
to move, the policy vector, how the global `random` state was prepared (seed, number of getrandbits(32) calls), the move
the reference returned and the state it left (position + sha256 of the 624 key words).  The label letters are those of the
categories the tests require (see CATEGORIES)."""
import argparse
import hashlib
import io
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")

CATEGORIES = {
    "a": "a ko point that is forbidden",
    "b": "a point forbidden only by superko",
    "c": "a position right after a pass",
    "d": "PASS is the only survivor of the cut",
    "e": "exactly one on-board survivor",
    "f": "an illegal point carries the maximal policy",
    "g": "candidates one float32 ulp above and below max * 0.1",
    "h": "policy entries equal to 0",
    "i": "an odd stream position",
    "j": "a draw that crosses the 624-word boundary",
}


def orchestrate():
    ref = os.environ.get("TAMAGO_REFERENCE")
    if not ref or not os.path.isdir(ref):
        print("set TAMAGO_REFERENCE to a checkout of the reference - nothing to do")
        return 1
    os.makedirs(GOLD, exist_ok=True)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    for size in (9, 13, 19):
        scratch = tempfile.mkdtemp(prefix=f"ref{size}_")
        try:
            tree = os.path.join(scratch, "ref")
            shutil.copytree(ref, tree, ignore=shutil.ignore_patterns(".git", "__pycache__"))
            path = os.path.join(tree, "board", "constant.py")
            text = open(path, encoding="utf-8").read().replace("BOARD_SIZE = 9", f"BOARD_SIZE = {size}")
            open(path, "w", encoding="utf-8").write(text)
            env["PYTHONPATH"] = tree + os.pathsep + REPO
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--size", str(size)], env=env, cwd=scratch)
        finally:
            shutil.rmtree(scratch, ignore_errors=True)
    return 0


def state_digest(state):
    words = np.asarray(state[1][:624], dtype=np.uint32)
    return int(state[1][624]), hashlib.sha256(words.tobytes()).hexdigest()


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as archive:
        for name, array in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(array), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            archive.writestr(info, buf.getvalue())


def softmax32(rs, n, temperature):
    z = rs.standard_normal(n) * temperature
    e = np.exp(z - z.max())
    return (e / e.sum()).astype(np.float32)


def worker(size: int):
    import torch

    from board.constant import BOARD_SIZE, PASS
    assert BOARD_SIZE == size, (BOARD_SIZE, size)
    from board.go_board import GoBoard
    from board.stone import Stone
    from nn.policy_player import generate_move_from_policy

    W, P = size + 2, size * size
    A = P + 1

    def at(x, y):
        return x + y * W

    class Stub:
        """A network object whose inference returns the vectors it was given, one per call."""
        def __init__(self, vectors):
            self.vectors = list(vectors)
            self.calls = 0

        def inference(self, _planes):
            vec = self.vectors[self.calls]
            self.calls += 1
            return torch.tensor(np.asarray(vec, dtype=np.float32)[None]), torch.zeros((1, 3))

    def replay(moves, superko):
        board = GoBoard(board_size=size, check_superko=superko)
        color = Stone.BLACK
        for pos in moves:
            board.put_stone(pos, color)
            color = Stone.get_opponent_color(color)
        return board, color

    def index_of(board, pos):
        return board.onboard_pos.index(pos)

    # black (2,1) (1,2) (2,3) (3,2), white (3,1) (4,2) (3,3), then white takes at (2,2): black may not retake at (3,2)
    ko = [at(2, 1), at(3, 1), at(1, 2), at(4, 2), at(2, 3), at(3, 3), at(3, 2), at(2, 2)]
    ko_point = at(3, 2)
    rs = np.random.RandomState(1000 + size)
    walk = random.Random(2000 + size)

    def random_moves(n, superko, pass_rate=0.05):
        board = GoBoard(board_size=size, check_superko=superko)
        color = Stone.BLACK
        moves = []
        for _ in range(n):
            legal = [p for p in board.onboard_pos if board.is_legal_not_eye(p, color)]
            pos = PASS if not legal or walk.random() < pass_rate else walk.choice(legal)
            board.put_stone(pos, color)
            moves.append(pos)
            color = Stone.get_opponent_color(color)
        return moves

    cases = []

    def add(name, moves, superko, policy, seed, n_bits, made=""):
        cases.append({"name": name, "moves": [int(m) for m in moves], "superko": bool(superko),
                      "policy": np.asarray(policy, dtype=np.float32), "seed": int(seed), "n_bits": int(n_bits), "made": made})

    # -- constructed cases ---------------------------------------------------------------------------------------------
    pol = softmax32(rs, A, 1.0)
    board, _ = replay(ko, True)
    pol[index_of(board, ko_point)] = np.float32(0.6)                    # the forbidden ko point carries the maximum
    add("ko_forbidden", ko, True, pol, 11, 0)
    for superko in (True, False):                                          # after two passes the retake repeats a position
        pol = softmax32(rs, A, 1.5)
        pol[index_of(board, ko_point)] = np.float32(0.3)
        add(f"retake_after_passes_superko_{int(superko)}", ko + [PASS, PASS], superko, pol, 12, 1)
    moves = random_moves(size + 4, True, 0.0)
    pol = np.full(A, 1e-4, dtype=np.float32)
    pol[P] = np.float32(0.9)
    add("pass_only", moves, True, pol, 13, 2)
    pol = np.full(A, 1e-5, dtype=np.float32)
    board, color = replay(moves, True)
    legal = [p for p in board.onboard_pos if board.is_legal(p, color)]
    pol[index_of(board, legal[len(legal) // 2])] = np.float32(0.8)
    add("one_point", moves, True, pol, 14, 3)
    pol = np.full(A, 0.004, dtype=np.float32)                              # an occupied point has the maximum: the cut comes
    pol[index_of(board, moves[0])] = np.float32(0.5)                     # from the legal 0.04, so every 0.0045 survives
    pol[index_of(board, legal[0])] = np.float32(0.04)
    pol[[index_of(board, p) for p in legal[1:6]]] = np.float32(0.0045)
    add("illegal_maximum", moves, True, pol, 15, 0)
    pol = np.full(A, 0.01, dtype=np.float32)                               # one ulp either side of max * 0.1
    pol[index_of(board, legal[0])] = np.float32(0.5)
    pol[index_of(board, legal[1])] = np.float32(0.05)
    pol[index_of(board, legal[2])] = np.nextafter(np.float32(0.05), np.float32(0.0))
    pol[index_of(board, legal[3])] = np.float32(0.05)
    pol[P] = np.nextafter(np.float32(0.05), np.float32(0.0))
    for k, seed in enumerate((16, 17, 18)):
        add(f"ulp_pair_{k}", moves, True, pol, seed, k, made="g")
    pol = softmax32(rs, A, 2.0)
    pol[[index_of(board, p) for p in legal[::3]]] = np.float32(0.0)
    add("zeros", moves, True, pol, 19, 5)
    # -- stream positions: 624 (fresh seed), 622 (the draw just fits), 623 (it straddles the twist), odd ones ------------
    for n_bits in (0, 1, 622, 623, 624, 1247):
        add(f"stream_after_{n_bits}_words", random_moves(10 + n_bits % 7, False), False, softmax32(rs, A, 1.0), 20 + n_bits, n_bits)
    # -- positions of random play, softmaxes at several temperatures -----------------------------------------------------
    for k, temperature in enumerate((0.3, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 8.0)):
        superko = k % 2 == 0
        add(f"random_play_{k}", random_moves(int(P * (0.2 + 0.1 * k)), superko, 0.08), superko, softmax32(rs, A, temperature),
            100 + k, k % 3)

    # -- the reference's answers ----------------------------------------------------------------------------------------
    records = []
    for case in cases:
        board, color = replay(case["moves"], case["superko"])
        plain, _ = replay(case["moves"], False)
        pol = case["policy"]
        legal = [p for p in board.onboard_pos if board.is_legal(p, color)]
        legal_plain = [p for p in plain.onboard_pos if plain.is_legal(p, color)]
        weights = [float(pol[index_of(board, p)]) for p in legal] + [float(pol[P])]
        cut = max(weights) * 0.1
        survivors = [p for p, w in zip(legal + [PASS], weights) if w > cut]
        random.seed(case["seed"])
        for _ in range(case["n_bits"]):
            random.getrandbits(32)
        start = int(random.getstate()[1][624])
        stub = Stub([pol])
        move = generate_move_from_policy(stub, board, color)
        assert stub.calls == 1 and move in survivors
        pos_after, sha = state_digest(random.getstate())
        labels = set(case["made"])
        _, prev, _ = board.record.get(board.moves - 1)
        if board.ko_move == board.moves - 1 and board.ko_pos not in legal and board.ko_pos in board.onboard_pos:
            labels.add("a")
        if legal != legal_plain:
            labels.add("b")
        if board.moves > 1 and prev == PASS:
            labels.add("c")
        if survivors == [PASS]:
            labels.add("d")
        if len([p for p in survivors if p != PASS]) == 1:
            labels.add("e")
        top = int(np.argmax(pol))
        if top < P and board.onboard_pos[top] not in legal:
            labels.add("f")
        if any(pol[index_of(board, p)] == 0 for p in legal):
            labels.add("h")
        if start % 2 == 1:
            labels.add("i")
        if start == 623:
            labels.add("j")
        records.append({"name": case["name"], "moves": case["moves"], "superko": case["superko"], "color": int(color.value),
                        "seed": case["seed"], "n_bits": case["n_bits"], "start_pos": start, "labels": sorted(labels),
                        "move": int(move), "state_pos": pos_after, "state_sha256": sha})
    seen = set().union(*(r["labels"] for r in records))
    assert seen == set(CATEGORIES), f"categories without a case at {size}x{size}: {sorted(set(CATEGORIES) - seen)}"
    out = {"size": size, "categories": CATEGORIES, "cases": records}
    arrays = {"policy": np.stack([c["policy"] for c in cases])}

    # -- the engine mode: the reference's command loop with policy_move=True -----------------------------------------------
    if size == 9:
        import gtp.client as ref_client
        from mcts.time_manager import TimeControl
        script = ("boardsize 9\nclear_board\ngenmove b\ngenmove w\ngenmove b\ngenmove w\nplay b pass\ngenmove w\n"
                  "genmove b\ngenmove w\nquit\n")
        vectors = [softmax32(rs, A, 1.0 + 0.5 * k) for k in range(7)]
        stub = Stub(vectors)
        ref_client.load_network = lambda model_file_path, use_gpu: stub
        client = ref_client.GtpClient(9, True, "stub", False, True, False, 7.0, TimeControl.CONSTANT_PLAYOUT, 10, 5.0, 0.0,
                                      1, 64, False, 0.0, 0.0)
        random.seed(77)
        random.getrandbits(32)
        old_in, old_out = sys.stdin, sys.stdout
        sys.stdin, sys.stdout = io.StringIO(script), io.StringIO()
        try:
            try:
                client.run()
            except (SystemExit, EOFError):
                pass
            stdout = sys.stdout.getvalue()
        finally:
            sys.stdin, sys.stdout = old_in, old_out
        assert stub.calls == 7
        pos_after, sha = state_digest(random.getstate())
        out["gtp"] = {"script": script, "seed": 77, "n_bits": 1, "stdout": stdout, "state_pos": pos_after, "state_sha256": sha}
        arrays["gtp_policy"] = np.stack(vectors)

    save_npz(os.path.join(GOLD, f"policy_moves_s{size}.npz"), arrays)
    with open(os.path.join(GOLD, f"policy_moves_s{size}.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(size, len(records), "cases;", {k: sum(k in r["labels"] for r in records) for k in sorted(CATEGORIES)})


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--size", type=int, default=0)
    args = parser.parse_args()
    sys.exit(worker(args.size) or 0 if args.size else orchestrate())
