#!/usr/bin/env python3
"""Generate tests/golden/vqtts_model_keys.json: the state-dict key -> shape map of THE REFERENCE's own `VQTTS`
(models/vqtts/vqtts.py:16-107), constructed on the CPU at the test configuration of tests/vqtts_model_helpers.py.  A list of
names and shapes, no weights.  The harness of make_golden.py is reused (its import sets up the paths, the working directory
and the stand-ins), and the text front end is stubbed as in make_golden_glow_infer.py: `CMUDictParser` needs inflect /
unidecode and a dictionary file, so an in-memory `models.parser` whose parser is None stands in.  Nothing of the reference
is changed.  Run from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vqtts_model.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
import make_golden as mg  # noqa: E402  (REF first on sys.path, cwd = REF, librosa / np.bool stand-ins)

import numpy as np  # noqa: E402
import types  # noqa: E402

sys.path.insert(0, os.path.join(mg.REPO, "tests"))
import vqtts_model_helpers as H  # noqa: E402


def main():
    if not hasattr(np, "bool"):
        np.bool = bool
    parser = types.ModuleType("models.parser")
    parser.CMUDictParser = lambda path: None
    sys.modules.setdefault("models.parser", parser)
    import models.vqtts.vqtts as ref_vqtts
    model = ref_vqtts.VQTTS(mg.wrap(H.config_dict()))
    keys = {k: list(v.shape) for k, v in model.state_dict().items()}
    path = os.path.join(mg.OUT, "vqtts_model_keys.json")
    with open(path, "w") as f:
        json.dump(keys, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote vqtts_model_keys.json: {len(keys)} keys ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
