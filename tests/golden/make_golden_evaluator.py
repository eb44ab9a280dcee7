#!/usr/bin/env python3
"""Records what hmd_ego_pose_amd/evaluate.py refuses and what its folder readers read, for the tests that hold later versions to it:

  evaluator_refusals.json   case -> [exception type, message] of tests/test_evaluator_refusals_cpu.py's case list
  folder_readers.npz        reader|attribute -> value of tests/test_folder_readers_cpu.py's readers

The committed files were written on the commit BEFORE ``DeviceEvaluator`` / ``SceneEvaluator`` got their common core and the two
readers their common part (the case list and the readers use public names only, so they run there unchanged).  Running it again
overwrites them with what the checked-out code does - do that only to record an intended change.  No GPU.

    python tests/golden/make_golden_evaluator.py
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    from tests import test_evaluator_refusals_cpu as R
    from tests import test_folder_readers_cpu as F
    with tempfile.TemporaryDirectory() as tmp:
        folders = R.make_folders(os.path.join(tmp, "refusals"))
        refusals = {name: R.run_case(name, folders) for name in sorted(R.CASES)}
        readers = F.record(os.path.join(tmp, "readers"))
    with open(os.path.join(HERE, "evaluator_refusals.json"), "w") as f:
        json.dump(refusals, f, indent=0, sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "folder_readers.npz"), **readers)
    print(f"{len(refusals)} refusals, {len(readers)} reader attributes")


if __name__ == "__main__":
    main()
