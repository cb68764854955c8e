"""Helper of test_gpu_search_plan.py (run as a script: most selection knobs are read once per process).  Creates search
handles - nothing else is launched - and prints, as one JSON line, the device's CU count and tg_search_launch_name of the
three families for each of them."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HANDLES = ((9, 1), (9, 17), (9, 300), (13, 2), (19, 2))
TREE_SIZE, BATCH = 64, 8


def main():
    import torch
    from tamago_amd import lib as tl
    lib = tl.load()

    def names(handle):
        out = {}
        buf = ctypes.create_string_buffer(160)
        for key, family, max_n, unique in (("puct", 0, BATCH, 0), ("gumbel", 1, BATCH, 0), ("gumbel_unique", 1, BATCH, 1),
                                           ("gumbel_513", 1, 513, 1), ("backup", 2, 0, 0), ("backup_unique", 2, 0, 1)):
            tl.check(lib.tg_search_launch_name(handle, family, max_n, unique, buf, len(buf)), "tg_search_launch_name")
            out[key] = buf.value.decode()
        return out

    res = {"cus": torch.cuda.get_device_properties(0).multi_processor_count, "handles": {}}
    for S, T in HANDLES:
        cfg = tl.SearchConfig(S, T, TREE_SIZE, BATCH, 0, 0, 0, 0)
        handle = ctypes.c_void_p()
        tl.check(lib.tg_search_create(ctypes.byref(cfg), ctypes.byref(handle)), "tg_search_create")
        entry = {"plain": names(handle)}
        if (S, T) == (9, 1):
            tl.check(lib.tg_search_profile(handle, 1, None), "tg_search_profile")
            entry["profile"] = names(handle)
            tl.check(lib.tg_search_profile(handle, 0, None), "tg_search_profile")
            os.environ["TG_GUMBEL_ONE_BY_ONE"] = "1"          # (read per call, TG_DEBUG_KNOBS=1: a kernel argument, no part of the choice)
            entry["one_by_one"] = names(handle)
            del os.environ["TG_GUMBEL_ONE_BY_ONE"]
            entry["again"] = names(handle)
        tl.check(lib.tg_search_destroy(handle), "tg_search_destroy")
        res["handles"][f"{S},{T}"] = entry
    print("NAMES " + json.dumps(res))


if __name__ == "__main__":
    main()
