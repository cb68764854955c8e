"""Parameter blobs for the weight-image tests (test_net_weights_host.py, test_gpu_net_load_bits.py): built from numpy seeds,
never committed.  ``BLOBS`` names them; ``make_blob(name)`` -> (board size, flat float32 blob in state_dict_keys order)."""
import numpy as np

from tamago_amd.nn.network.dual_net import flatten_state, state_dict_keys


def random_state(board_size: int, seed: int):
    """conv / FC tensors U(+-1/sqrt(fan_in)), batch-norm weight and running_var U(0.5, 1.5), bias and running_mean N(0, 0.1)."""
    rs = np.random.RandomState(seed)
    state = {}
    for key, shape in state_dict_keys(board_size):
        leaf = key.split(".")[-1]
        if "bn" in key.split(".")[-2]:
            v = rs.uniform(0.5, 1.5, size=shape) if leaf in ("weight", "running_var") else rs.normal(0.0, 0.1, size=shape)
        else:
            if leaf == "weight":
                fan_in = int(np.prod(shape[1:]))
            else:                                  # FC bias: fan_in of the matching weight
                fan_in = (2 if key.startswith("policy") else 1) * board_size ** 2
            v = rs.uniform(-1.0, 1.0, size=shape) / np.sqrt(fan_in)
        state[key] = v.astype(np.float32)
    return state


def _zeros(state):
    state["blocks.2.conv1.weight"][:] = 0.0                      # mx == 0: exponent 0, and a layer without a spread
    state["policy_head.fc_layer.weight"][:] = 0.0


def _spread(state):
    state["blocks.1.conv2.weight"][:, 5] *= np.float32(2.0 ** -12)   # one input channel far below the others
    state["conv_layer.weight"] *= np.float32(2.0 ** 20)              # a negative exponent


def _spread_wide(state):
    state["blocks.4.conv1.weight"][:, 40] *= np.float32(2.0 ** -20)  # beyond the direct split family's limit (2^18) too


def _tiny(state):
    for key in state:
        if "conv" in key:
            state[key] *= np.float32(2.0 ** -60)                 # exponent above 70: clamped to 40 in w1d and heads, not in split


def _nonfinite(state):
    w = state["blocks.3.conv1.weight"]
    w[3, 7, 1, 1] = np.nan
    w[20, 7, 0, 2] = np.inf
    w[41, 30, 2, 0] = -np.inf


# name -> (board size, seed, edit of the random state)
BLOBS = {
    "s9": (9, 901, None),
    "s13": (13, 1301, None),
    "s19": (19, 1901, None),
    "s9_zeros": (9, 902, _zeros),
    "s9_spread": (9, 903, _spread),
    "s9_spread_wide": (9, 906, _spread_wide),
    "s9_tiny": (9, 904, _tiny),
    "s9_nonfinite": (9, 905, _nonfinite),
}


def make_state(name: str):
    size, seed, edit = BLOBS[name]
    state = random_state(size, seed)
    if edit:
        edit(state)
    return size, state


def make_blob(name: str):
    size, state = make_state(name)
    return size, flatten_state(state, size)
