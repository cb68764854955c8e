#!/usr/bin/env python3
"""Record the tree digests of tests/_select_rcp_digest.py CASES into tests/golden/select_rcp_digests.json (GPU needed).

The recorded trees are those of the one-wavefront kernel (TG_SELECT_SERIAL=1): IEEE divisions and __dsqrt_rn, every node read
from the pool at every step.  tests/test_gpu_select_rcp.py holds every selection kernel to these digests, so an error common
to the kernels of one build cannot hide behind a comparison among them.  Recorded at commit 38f7062.
    python tools/gen_golden_select_rcp.py [--check]        (--check: compare with the committed file instead of writing it)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _select_rcp_digest import CASES  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "select_rcp_digests.json")
SCRIPT = os.path.join(ROOT, "tests", "_select_rcp_digest.py")


def main():
    env = dict(os.environ, TG_DEBUG_KNOBS="1", TG_SELECT_SERIAL="1", TG_SELECT_SPLIT="0")
    env.pop("TG_SELECT_MPIPE_TREES", None)
    got = {}
    for name, cfg in CASES.items():
        res = subprocess.run([sys.executable, SCRIPT] + cfg.split(), env=env, capture_output=True, text=True, timeout=600)
        if res.returncode != 0:
            sys.exit(f"{name}: exit {res.returncode}\n{res.stderr[-2000:]}")
        digest, nodes, root_visits = res.stdout.strip().splitlines()[-1].split()
        got[name] = {"argv": cfg, "digest": digest, "nodes": int(nodes), "max_root_visits": int(root_visits)}
        print(name, got[name], flush=True)
    if "--check" in sys.argv:
        with open(OUT) as f:
            want = json.load(f)
        sys.exit(0 if want == got else f"digests differ from {OUT}")
    with open(OUT, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
