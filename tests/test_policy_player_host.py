"""Host side of the policy player (tamago_amd/nn/policy_player.py) against moves recorded from the reference's own
generate_move_from_policy (nn/policy_player.py:13-46) and its GTP engine mode (gtp/client.py:206-211)."""
import io
import random

import numpy as np
import pytest
import torch

from _policy_cases import CATEGORIES, digest, load, prepared_rng, replay


class _Recorded:
    """A network object whose inference returns recorded vectors, one per call."""

    def __init__(self, vectors):
        self.vectors = list(vectors)
        self.calls = 0

    def inference(self, planes):
        vec = self.vectors[self.calls]
        self.calls += 1
        assert tuple(planes.shape[:2]) == (1, 6)
        return torch.tensor(np.asarray(vec, dtype=np.float32)[None]), torch.zeros((1, 3))


@pytest.mark.parametrize("size", [9, 13, 19])
def test_choose_from_policy_reproduces_the_reference(size):
    from tamago_amd.nn.policy_player import choose_from_policy
    labels, arrays = load(size)
    cases = labels["cases"]
    assert len(cases) == len(arrays["policy"]) >= 20
    seen = set()
    for case, policy in zip(cases, arrays["policy"]):
        board, color = replay(size, case)
        rng = prepared_rng(case)
        move = choose_from_policy(policy, board, color, rng)
        assert move == case["move"], case["name"]
        assert digest(rng.getstate()[1]) == (case["state_pos"], case["state_sha256"]), case["name"]
        seen.update(case["labels"])
    assert seen == set(CATEGORIES)


def test_generate_move_from_policy_uses_the_global_generator():
    """A network that is no DualNet: inference + choose_from_policy on the `random` module's own state."""
    from tamago_amd.nn.policy_player import generate_move_from_policy
    labels, arrays = load(9)
    for case, policy in list(zip(labels["cases"], arrays["policy"]))[:8]:
        board, color = replay(9, case)
        random.setstate(prepared_rng(case).getstate())
        net = _Recorded([policy])
        assert generate_move_from_policy(net, board, color) == case["move"], case["name"]
        assert net.calls == 1
        assert digest(random.getstate()[1]) == (case["state_pos"], case["state_sha256"]), case["name"]


def test_gtp_policy_move_session():
    """GtpClient(policy_move=True): the recorded session of the reference's command loop, byte for byte - the moves drawn
    from the policies, a pass answered with a pass, and the global generator left where the reference leaves it."""
    from tamago_amd.gtp.client import GtpClient
    labels, arrays = load(9)
    session = labels["gtp"]
    net = _Recorded(arrays["gtp_policy"])
    out = io.StringIO()
    client = GtpClient(9, True, net, policy_move=True, stdin=io.StringIO(session["script"]), stdout=out)
    random.seed(session["seed"])
    for _ in range(session["n_bits"]):
        random.getrandbits(32)
    client.run()
    assert out.getvalue() == session["stdout"]
    assert net.calls == len(arrays["gtp_policy"])
    answers = [block.strip() for block in out.getvalue().split("\n\n") if block.strip()]
    script = session["script"].split("\n")
    after_pass = script.index("play b pass") + 1
    assert script[after_pass] == "genmove w" and answers[after_pass] == "= pass"
    assert digest(random.getstate()[1]) == (session["state_pos"], session["state_sha256"])


def test_seed_states_are_pythons():
    """tg_policy_seed_states (host arithmetic of the library) against random.Random(seed).getstate()."""
    from tamago_amd import build
    from tamago_amd.nn.policy_player import seed_states
    build.build(verbose=False)
    seeds = [0, 1, 2, 77, 300, 65536, 123456789, 2 ** 31, 2 ** 32 - 1] + list(range(1000, 1040))
    got = seed_states(seeds)
    for seed, words in zip(seeds, got):
        assert tuple(int(w) for w in words) == random.Random(seed).getstate()[1], seed
    big = seed_states([2 ** 40, -5])                      # outside the one-word range: through Random itself
    assert tuple(int(w) for w in big[0]) == random.Random(2 ** 40).getstate()[1]
    assert tuple(int(w) for w in big[1]) == random.Random(-5).getstate()[1]
