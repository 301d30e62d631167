#!/usr/bin/env python3
"""How nested_fit_entries.npz and nested_fit_workspace_bytes.json were recorded: from the build of commit 497521c, the last one in which the three
one-call fit entries each had their own host chain.  Run from a checkout root of that commit (with the two test modules copied into tests/):

    python tests/golden/make_golden_nested_fit_entries.py             # both files; the .npz needs an MI355X
    python tests/golden/make_golden_nested_fit_entries.py --cpu       # the workspace sizes only

Every case is called five times; the script refuses to write unless the five results are identical bytes (the tests compare exactly)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from gabotorch_amd import _lib                                        # noqa: E402
from tests import test_nested_fit_entries_cpu as cpu                  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    with open(os.path.join(HERE, "nested_fit_workspace_bytes.json"), "w") as fh:
        json.dump(cpu._grid(_lib.load()), fh, indent=0, sort_keys=True)
        fh.write("\n")
    if "--cpu" in sys.argv:
        return
    from tests import test_gpu_nested_fit_entries as gpu
    store = {}
    for case in gpu.CASES:
        for g in (1, 0):
            runs = [gpu.evaluate(case, g) for _ in range(5)]
            assert all(rc == _lib.GABO_OK and out.tobytes() == runs[0][1].tobytes() for rc, out in runs), (case, g)
            store[f"{gpu.case_id(case)}-g{g}"] = runs[0][1]
    for case in gpu.NPD_CASES:
        runs = [gpu.evaluate(case, 1, noise=gpu.NPD_NOISE) for _ in range(5)]
        assert all(rc == _lib.GABO_OK and out[5] == runs[0][1][5] for rc, out in runs), case
        store[f"{gpu.case_id(case)}-npd"] = runs[0][1][5:6].copy()
    np.savez_compressed(os.path.join(HERE, "nested_fit_entries.npz"), **store)


if __name__ == "__main__":
    main()
